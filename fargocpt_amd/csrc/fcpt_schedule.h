// Chunk planner of the marching kernels: how many rings every wavefront of k_source_march* and k_transport_fused
// gets, per grid and per device size.  Host arithmetic only (fcpt_schedule.cpp includes no HIP header); the number of
// compute units is an argument, queried once by the HIP unit (device_cus(), fcpt_kernels.h).
#ifndef FCPT_SCHEDULE_H
#define FCPT_SCHEDULE_H

#include <vector>

#include "fcpt_internal.h"

// Tile and chunk geometry that the kernels and the planner share.
#define MARCH_VALID 59 /* columns a wavefront of the marching source kernels stores (kernels/source_march.h) */
#define TF_XCD_CHUNKS 16 /* launches of at least this many chunks deal whole chunks to the XCDs */
#define TF_HALO_LO 5 /* cells of a 64-column segment that are not final: left ... */
#define TF_HALO_HI 6 /* ... and right */
#define TF_STRIDE (64 - TF_HALO_LO - TF_HALO_HI) /* columns a wavefront stores: tiles of 53 */
#define RADIAL_ROWS 16 /* rings per thread on grids that fill the GPU; fewer on small ones (march_len) */
#define THETA_ROWS 8
#define CFL_ROWS 8 /* on grids that fill the GPU; fewer on small ones (march_len) */

namespace fcpt {

inline int tiles_of(int nphi) { return (nphi + TF_STRIDE - 1) / TF_STRIDE; }       // of k_transport_fused
inline int segments_of(int nphi) { return (nphi + MARCH_VALID - 1) / MARCH_VALID; } // of the marching source kernels

// n_cu: compute units of the device
int march_len(const Dev &P, int n_cu, int rows_full);
int source_rows(const Dev &P, int n_cu);
int transport_rows(const Dev &P, int n_cu);
std::vector<int> source_schedule(const Dev &P, int n_cu);
std::vector<int> source_schedule_explicit(const Dev &P, const std::vector<int> &lengths, bool *refused);
std::vector<int> transport_schedule(const Dev &P, int n_cu, const std::vector<int> &slow_rings, const std::vector<int> *lengths);
bool transport_can_split(const Dev &P, int n_cu, bool shear_safe);
bool source_march_applies(const Dev &P);
// test hook (no GPU needed): the two tables for a grid, an EOS and a device of n_cu compute units; the first
// damp_inner and the last damp_outer rings load reference values in the transport (damping zones)
void selftest_chunk_tables(int nr, int nphi, int n_cu, int adiabatic, int damp_inner, int damp_outer, const Options &opt,
                           std::vector<int> &transport, std::vector<int> &source);

} // namespace fcpt
#endif
