// fargocpt_hip -- the host driver's shared declarations: one small header for its translation units
// (config.cpp, bodies.cpp, particles.cpp, output.cpp, run.cpp, main.cpp).  Host code over the C ABI only.
#pragma once
#include "../../../include/fargocpt_hip.h"

#include <array>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <map>
#include <string>
#include <vector>

#define CHECK(call)                                                                      \
    do {                                                                                 \
        const int rc_ = (call);                                                          \
        if (rc_ != FCPT_OK) {                                                            \
            fprintf(stderr, "fargocpt_hip: %s failed (%d): %s\n", #call, rc_, fcpt_last_error()); \
            exit(1);                                                                     \
        }                                                                                \
    } while (0)

// ---- config.cpp: the YAML setup, the code units, the descriptor ----------------------------------------------------
std::string lower(std::string s);

// "key: value  # comment" lines and one list of maps ("nbody:"), which is all the reference's
// setups use (src/config.cpp wraps yaml-cpp; keys are case-insensitive, :344-349).
struct Config {
    std::map<std::string, std::string> kv;
    std::vector<std::map<std::string, std::string>> nbody;
    mutable std::map<std::string, bool> used;

    bool load(const std::string &path);
    bool has(const std::string &k) const { return kv.count(lower(k)) > 0; }
    std::string str(const std::string &k, const std::string &def) const;
    bool flag(const std::string &k, bool def) const;
};

// code units (set_baseunits, src/units.cpp:131-185): l0 and m0 from the setup (default 1 au, 1 solMass), time and
// temperature units derived with G = 1 and R_gas = 1.  config_to_desc fills it.
const double G_CGS = 6.67430e-8, KB = 1.380649e-16, MU = 1.66053906660e-24;
const double AU_CM = 1.495978707e13, SOLMASS_G = 1.988409870698051e33;
struct Units {
    double L0 = AU_CM, M0 = SOLMASS_G;
    double TEMP0 = G_CGS * MU / KB * M0 / L0;
    double TIME0 = std::sqrt(L0 * L0 * L0 / (G_CGS * M0));
};

// "<number> [unit]" -> code units for the quantity kind; a unit that is not understood exits with 2
enum Kind { K_NONE, K_LEN, K_MASS, K_SIGMA, K_TEMP, K_VISC, K_DENS };
double number(const Units &u, const std::string &s, Kind kind);
double num(const Config &c, const Units &u, const std::string &k, double def, Kind kind = K_NONE);

void config_to_desc(const Config &c, fcpt_desc &d, Units &u);
// exit_on_unknown_key of the reference, then the features outside the gas path that the setup switches on
void check_keys(const Config &c, bool lenient, bool master);
void note_unused_keys(const Config &c);

// Dust particles: the Particle* keys of parameters.cpp:853-961 with their units and defaults
struct ParticleSetup {
    bool on = false, cartesian_gravity = false;
    bool gas_drag = true, diffusion = false; // ParticleGasDragEnabled, ParticleDustDiffusion (with --dust-seed)
    bool calculate_disk = true;              // parameters::calculate_disk: Disk: No freezes the gas under the particles
    long n = 0;
    int species = 1;
    double radius = 0, radius_factor = 10, eccentricity = 0, density = 0, slope = 0;
    double rmin = 0, rmax = 0, escape_min = 0, escape_max = 0;
};
// the Particle* keys, and the refusals (exit 2) of what the library's particle step does not cover
ParticleSetup read_particle_setup(const Config &c, const Units &u, const fcpt_desc &d, bool have_dust_seed, bool several_ranks);

// Self-gravity of the gas: SelfGravity with SelfGravityMode: basic | symmetric (parameters.cpp:698-728)
struct SelfGravitySetup {
    bool on = false;
    int mode = FCPT_SG_OFF;
    double aspect_ratio = 0, thickness_smoothing_sg = 0;
    bool write_rad = false, write_azi = false; // WriteSGAccelRad / WriteSGAccelAzi
    bool indirect_disk = false;                // IndirectTermDiskOnDisk (auto: yes with self-gravity)
};
// the keys, and the refusals (exit 2) of what the library's solver does not cover
SelfGravitySetup read_selfgravity_setup(const Config &c, const Units &u, const fcpt_desc &d, bool several_ranks);

struct Body {
    double a, m, phase, rsm_factor;
    double rampup; // "ramp-up time" in orbital periods (planet.cpp:166-179)
    double ecc = 0.0, pericenter = 0.0, true_anomaly = 0.0; // --bodies free (planetary_system.cpp:172-189)
};
std::vector<Body> read_bodies(const Config &c, const Units &u, const fcpt_desc &d);

// ---- output.cpp ----------------------------------------------------------------------------------------------------
// This process's slab: rank, the rows of the global grid it holds and the window of them it writes
// (Zero_or_active / Max_or_active, src/split.cpp:66-78)
struct Slab {
    int rank = 0, nranks = 1;
    fcpt_split s;
    int nphi = 0, nr_global = 0;
    bool master() const { return rank == 0; }
    bool multi() const { return nranks > 1; }
    size_t local_count(bool vec) const { return (size_t)(s.nr + (vec ? 1 : 0)) * nphi; }
    // rows [lo, hi) of the local grid that write2D / write1D store, at global row imin + lo: the overlap rings are
    // stripped, and only the last slab writes the last interface row of a vector grid (polargrid.cpp:150-172)
    void window(bool vec, int &lo, int &hi) const
    {
        lo = s.zero_or_active;
        hi = s.max_or_active + ((vec && s.is_last) ? 1 : 0);
    }
};

// What every stage after the descriptor works on
struct Driver {
    fcpt_ctx *ctx = nullptr;
    fcpt_desc desc;
    Units units;
    Slab slab;
    std::vector<double> radii; // interface radii of the global grid (fcpt_radii)
    std::string outdir, cfgpath;
    bool quiet = false;
    SelfGravitySetup sg;
};

void mkdirs(const std::string &p);
// fopen that prints "fargocpt_hip: cannot write <path>" (modes w, a) or "cannot read <path>" and exits with 1
[[noreturn]] void die_cannot(const char *verb, const std::string &path);
FILE *open_or_die(const std::string &path, const char *mode);
void barrier(const Driver &dr);
void exchange(const Driver &dr); // CommunicateBoundaries (commbound.cpp:98-182): returns at once for a single slab
double calc_dt(const Driver &dr);

struct BodySystem;
struct Particles;
bool needs_reference(const fcpt_desc &d);
void write_static_files(const Driver &dr);
// one snapshot directory: snapshots/<nsnap>/, or snapshots/<name>/ (the "reference" of the damping data)
void write_snapshot(const Driver &dr, const BodySystem &bs, Particles &pt, unsigned nsnap, unsigned nmon, const char *name);
struct misc_entry { // src/output.h:16-24
    unsigned int timestep;
    unsigned int nTimeStep;
    double time;
    double OmegaFrame;
    double FrameAngle;
    double last_dt;
    unsigned long int N_iter;
};
misc_entry restart_load(const Driver &dr, BodySystem &bs, Particles &pt, const std::string &restart_dir);

// ---- bodies.cpp: star and planets, on circular orbits or (--bodies free) as a system of their own ------------------
struct BodySystem {
    const Driver *dr = nullptr;
    std::vector<Body> bodies;
    bool free = false, disk_feedback = true;
    bool indirect = true; // HydroFrameCenter: primary (or all with a single body): the star-centred frame
    bool no_star_smoothing = false, smoothing_planetloc = false;
    fcpt_nbody *nb = nullptr; // every rank its own bit-identical copy
    // since the last monitor row: sum of m (x a_y - y a_x) dt of the disk's force on the body, and of the disk's indirect
    // term (minus its force on the star), as t_planet accumulates them (frame_of_reference.cpp:95-108)
    std::vector<double> torque_acc, indirect_acc;
    double itx = 0.0, ity = 0.0; // the indirect term of the step being set up: the particles feel it too

    int count() const { return (int)bodies.size(); }
    void init(const Config &c);
    double omega_kepler(const Body &b) const;
    double rampup_mass(const Body &b, double t, double m) const;
    double roche_smoothing(const Body &b) const;
    void set(double t) { free ? set_free(t, 0.0, nullptr, nullptr) : set_circular(t, 0.0); } // bodies to the context, no step
    void set_circular(double t, double dt);
    void queue_disk_force();
    void collect_disk_force(double *ax, double *ay);
    void set_free(double t, double dt, const double *ax, const double *ay);
    void advance(double dt);
    void correct_velocity_for_disk();
    void write_rows(unsigned nsnap, unsigned nmon, double t, bool create);
    void save(const std::string &dir) const; // <dir>nbody.bin
    void load(const std::string &dir);
};

// ---- particles.cpp -------------------------------------------------------------------------------------------------
// one record of snapshots/<n>/particles.dat: t_particle (particles/particle.h), 96 bytes
struct ParticleRecord {
    uint64_t id;
    double r, phi, r_dot, phi_dot, r_ddot, phi_ddot, mass, radius, timestep, facold, stokes;
};
static_assert(sizeof(ParticleRecord) == 96, "the reference's particle record");

struct Particles {
    const Driver *dr = nullptr;
    ParticleSetup ps;
    fcpt_particle_params prm;
    // mass, initial speed (r_ddot) and eccentricity (phi_ddot) of the record never change: kept here by id
    std::map<uint64_t, std::array<double, 3>> fixed;

    void init();
    void upload(const std::vector<ParticleRecord> &rec);
    std::vector<ParticleRecord> download();
    void place_initial();
    void write(const std::string &dir); // <dir>particles.dat
    void read(const std::string &dir);
};

// ---- run.cpp: main.cpp:117-152 and sim::run (simulation.cpp:505-558) -----------------------------------------------
struct Run {
    const Driver *dr = nullptr;
    BodySystem *bs = nullptr;
    Particles *pt = nullptr;
    long max_steps = -1;
    bool moving = false; // bodies or particles that need the host every step
    double time = 0.0, last_dt = 0.0;
    unsigned n_monitor = 0;
    unsigned long n_iter = 0, n_iter_last = 0;
    unsigned long n_iter_start = 0, n_in_run_steps = 0; // hydro steps of this run, and those taken inside fcpt_run_steps
    double sum_dt = 0, min_dt = 1e300, max_dt = 0;
    std::chrono::steady_clock::time_point t_start, t_last;
    FILE *tlog = nullptr;

    void begin(bool restarting, unsigned long long dust_seed);
    bool device_stretch();
    void host_step();
    void at_monitor();
    void loop();
    void finish();
};
