/*
 * fargocpt_hip.h -- C ABI of the MI355X-native FargoCPT gas update.
 *
 * The reference (kimweiskopf/fargocpt) has no FFI layer: its per-timestep gas
 * update is a set of free C++ functions over global state, called from
 * step_Euler (src/simulation.cpp:148-267).  This header is the boundary a
 * maintainer would bind instead of those calls; every entry point names the
 * reference function(s) it replaces.  Plain C types only: pointers, sizes,
 * doubles, int32.  One context per GPU / radial slab, one host thread per
 * context, all device work on one HIP stream (fcpt_set_stream).
 *
 * Field layout is the reference's t_polargrid::Field (src/polargrid.h:111-133):
 * row-major double[nr*nphi + naz], phi contiguous.  Scalar grids have Nr rows,
 * "vector" grids (v_radial, and tau_r_phi internally) have Nr+1 rows.
 *
 * All functions return 0 on success or a negative FCPT_E* code; no exceptions
 * cross the ABI.  fcpt_last_error() gives a human-readable message.
 */
#ifndef FARGOCPT_HIP_H
#define FARGOCPT_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define FCPT_ABI_VERSION 5

/* error codes */
#define FCPT_OK 0
#define FCPT_EINVAL -1  /* bad argument / unsupported configuration */
#define FCPT_ENOMEM -2  /* host or device allocation failed */
#define FCPT_EHIP -3    /* a HIP runtime call failed */
#define FCPT_ESPLIT -4  /* slab too narrow: needs >= 2*FCPT_OVERLAP rings (src/split.cpp:42-47) */
#define FCPT_ENODEV -5  /* no HIP device */
#define FCPT_ESHEAR -6  /* a step ran beyond the FARGO shear limit without its fallback (see fcpt_step) */
#define FCPT_ECOMM -7   /* an RCCL call failed, or librccl could not be loaded */

/* src/constants.h:17-19 */
#define FCPT_OVERLAP 7
#define FCPT_GHOSTCELLS_B 1
/* rows of geometry kept past the last local ring (src/init.cpp:40-45 search_buffer) */
#define FCPT_GEOM_PAD 15
#define FCPT_MAX_BODIES 8

/* enum-like int32 values of fcpt_desc ------------------------------------ */
enum { FCPT_SPACING_ARITHMETIC = 0, FCPT_SPACING_LOGARITHMIC = 1, FCPT_SPACING_EXPONENTIAL = 2 };
enum { FCPT_EOS_ISOTHERMAL = 0, FCPT_EOS_IDEAL = 1 };
enum { FCPT_ARTVISC_NONE = 0, FCPT_ARTVISC_TW = 1, FCPT_ARTVISC_SN = 2 };
enum { FCPT_LIMITER_VANLEER = 0, FCPT_LIMITER_MC = 1 };
enum { FCPT_OPACITY_LIN = 0, FCPT_OPACITY_BELL = 1, FCPT_OPACITY_CONST = 2, FCPT_OPACITY_SIMPLE = 3 };
enum { FCPT_BETAREF_ZERO = 0, FCPT_BETAREF_REFERENCE = 1, FCPT_BETAREF_MODEL = 2, FCPT_BETAREF_FLOOR = 3 };
enum { FCPT_INTEGRATOR_EULER = 0, FCPT_INTEGRATOR_LEAPFROG = 1 };
/* per-variable boundary conditions (src/boundary_conditions/config.cpp:97-343) */
enum {
    FCPT_BC_ZEROGRADIENT = 0,
    FCPT_BC_REFERENCE = 1,
    FCPT_BC_REFLECTING = 2, /* vrad only */
    FCPT_BC_OUTFLOW = 3,    /* vrad only */
    FCPT_BC_KEPLERIAN = 4,  /* vrad: keplerian_radial, vaz: keplerian_azimuthal */
    FCPT_BC_ZEROSHEAR = 5,  /* vaz only */
    FCPT_BC_NONE = 6
};
/* damping target (src/boundary_conditions/damping.cpp:152-178) */
enum { FCPT_DAMP_NONE = 0, FCPT_DAMP_REFERENCE = 1, FCPT_DAMP_ZERO = 2, FCPT_DAMP_MEAN = 3 };
/* initial condition generator (src/init.cpp:255-343) */
enum { FCPT_IC_PROFILE = 0, FCPT_IC_SPREADING_RING = 1, FCPT_IC_SHOCKTUBE = 2 };

/* grids addressable through upload / download / device_ptr
 * (subset of t_data::t_polargrid_type, src/data.h:17-86) */
enum {
    FCPT_F_SIGMA = 0,
    FCPT_F_VRAD = 1, /* (Nr+1) x Nphi */
    FCPT_F_VAZI = 2,
    FCPT_F_ENERGY = 3,
    FCPT_F_PRESSURE = 4,
    FCPT_F_SOUNDSPEED = 5,
    FCPT_F_SCALE_HEIGHT = 6,
    FCPT_F_VISCOSITY = 7,
    FCPT_F_TEMPERATURE = 8,
    FCPT_F_POTENTIAL = 9, /* ideal EOS, Euler: evaluated inside the source step; a download fills the grid from the current state */
    FCPT_F_SIGMA0 = 10,
    FCPT_F_VRAD0 = 11, /* (Nr+1) x Nphi */
    FCPT_F_VAZI0 = 12,
    FCPT_F_ENERGY0 = 13,
    FCPT_F_QPLUS = 14,
    FCPT_F_QMINUS = 15,
    /* VISCOSITY_CORRECTION_FACTOR_PHI|R (viscosity.cpp:256-348); only with StabilizeViscosity 1|2,
     * FCPT_EINVAL otherwise */
    FCPT_F_VISC_CFAC_PHI = 16,
    FCPT_F_VISC_CFAC_R = 17,
    /* MASSFLOW (src/data.h:76), (Nr+1) x Nphi, only with fcpt_desc.write_massflow: the mass every Transport()
     * carried through the inner interface of each cell, accumulated step by step as VanLeerRadial does for the
     * density (src/TransportEuler.cpp:609-616: "+= varq_inf").  The caller divides by the elapsed
     * Nmonitor * MonitorTimestep (quantities::calculate_massflow, src/quantities.cpp:770-781), sums over azimuth
     * for MassFlow1D.dat and clears the grid by uploading zeros (clear_after_write, src/data.cpp:277). */
    FCPT_F_MASSFLOW = 18,
    /* ACCEL_RADIAL / ACCEL_AZIMUTHAL (src/data.cpp:49-58), (Nr+1) x Nphi, only with BodyForceFromPotential: no: the
     * cell-centred acceleration of the gas by the bodies and the indirect term that CalculateAccelOnGas
     * (src/Pframeforce.cpp:96-189) left for the last source step (rows 0 and Nr are never written: zero) */
    FCPT_F_ACCEL_RADIAL = 19,
    FCPT_F_ACCEL_AZIMUTHAL = 20,
    /* SG_ACCEL_RAD / SG_ACCEL_AZI (src/data.cpp:61-68), Nr x Nphi, cell-centred: the acceleration of the gas by its own
     * gravity as the last fcpt_selfgravity_compute / _kick (or in-step kick) left it; only while fcpt_selfgravity is
     * switched on, FCPT_EINVAL otherwise */
    FCPT_F_SG_ACCEL_RAD = 21,
    FCPT_F_SG_ACCEL_AZI = 22,
    FCPT_F_COUNT = 23
};

/*
 * Everything the path reads from parameters::*, global.h and refframe:: in the
 * reference.  All lengths/times/masses are in code units (G = 1 by default).
 * The YAML key each member mirrors is given on the right
 * (src/parameters.cpp:520-900, src/Interpret.cpp:73-700,
 *  src/boundary_conditions/config.cpp, damping.cpp:185-271).
 */
typedef struct fcpt_desc {
    uint32_t struct_size; /* = sizeof(fcpt_desc), ABI check */
    uint32_t abi_version; /* = FCPT_ABI_VERSION */

    /* grid + radial slab decomposition (src/split.cpp:34-88) */
    int32_t nr_global; /* Nrad */
    int32_t nphi;      /* Naz */
    int32_t rank;      /* slab index, 0 = innermost */
    int32_t nranks;    /* number of slabs */
    int32_t radial_spacing; /* RadialSpacing */
    int32_t _pad0;
    double rmin, rmax;                   /* Rmin, Rmax */
    double exponential_cell_size_factor; /* ExponentialCellSizeFactor */

    /* equation of state */
    int32_t eos; /* EquationOfState */
    int32_t _pad1;
    double adiabatic_index; /* AdiabaticIndex */
    double mu;              /* mu */
    double aspect_ratio;    /* AspectRatio */
    double flaring_index;   /* FlaringIndex */
    double minimum_temperature, maximum_temperature; /* code units */

    /* disk profile / floors */
    double sigma0;      /* Sigma0 (code units) */
    double sigma_slope; /* SigmaSlope */
    double sigma_floor; /* SigmaFloor (multiples of sigma0) */

    /* viscosity */
    double viscous_alpha;           /* ViscousAlpha */
    double constant_viscosity;      /* ConstantViscosity */
    double radial_viscosity_factor; /* RadialViscosityFactor */
    int32_t stabilize_viscosity;    /* StabilizeViscosity: 0, 1 (damped viscous update) or 2 (dt limit) */
    int32_t artificial_viscosity;   /* ArtificialViscosity */
    double artificial_viscosity_factor;       /* ArtificialViscosityFactor */
    int32_t artificial_viscosity_dissipation; /* ArtificialViscosityDissipation */
    int32_t heating_viscous;                  /* HeatingViscous */
    double heating_viscous_factor;            /* HeatingViscousFactor */

    /* transport */
    int32_t fast_transport; /* Transport: FARGO=1 / standard=0 */
    int32_t flux_limiter;   /* FluxLimiter */

    /* time stepping */
    int32_t integrator; /* Integrator */
    int32_t _pad2;
    double cfl;                       /* CFL */
    double cfl_max_var;               /* CFLmaxVar */
    double first_dt;                  /* FirstDT */
    double heating_cooling_cfl_limit; /* HeatingCoolingCFLlimit */
    double monitor_timestep;          /* MonitorTimestep */
    int32_t nmonitor;                 /* Nmonitor */
    int32_t nsnapshots;               /* Nsnapshots */

    /* frame + gravity */
    double omega_frame;                /* OmegaFrame */
    double thickness_smoothing;        /* ThicknessSmoothing */
    int32_t body_force_from_potential; /* BodyForceFromPotential: 1 = gradient of the potential (CalculateNbodyPotential),
                                        * 0 = CalculateAccelOnGas (src/Pframeforce.cpp:96-189, SourceEuler.cpp:348-353,406-411) */
    int32_t _pad3;
    double hydro_center_mass; /* mass of the bodies defining the hydro centre */

    /* boundary conditions: [0] = inner, [1] = outer */
    int32_t bc_sigma[2];
    int32_t bc_energy[2];
    int32_t bc_vrad[2];
    int32_t bc_vaz[2];
    double keplerian_vaz_factor[2];  /* Inner/OuterBoundaryVaziKeplerianFactor */
    double keplerian_vrad_factor[2]; /* Inner/OuterBoundaryVradKeplerianFactor */

    /* wave damping */
    int32_t damping; /* Damping */
    int32_t _pad4;
    double damping_inner_limit;       /* DampingInnerLimit */
    double damping_outer_limit;       /* DampingOuterLimit */
    double damping_time_factor;       /* DampingTimeFactor */
    double damping_time_radius_outer; /* DampingTimeRadiusOuter */
    int32_t damp_vrad[2];   /* DampingVRadialInner/Outer */
    int32_t damp_vaz[2];    /* DampingVAzimuthalInner/Outer */
    int32_t damp_sigma[2];  /* DampingSurfaceDensityInner/Outer */
    int32_t damp_energy[2]; /* DampingEnergyInner/Outer */

    /* physical constants in code units (src/constants.cpp:236-262) */
    double G, Rgas, sigma_sb, c_light;

    /* initial conditions (src/init.cpp) */
    int32_t ic;                      /* ShockTube / SpreadingRing / profile */
    int32_t set_sigma0;              /* SetSigma0 */
    double disk_mass;                /* DiskMass */
    int32_t initialize_vradial_zero; /* InitializeVradialZero */
    int32_t initialize_pure_keplerian; /* InitializePureKeplerian */

    /* cooling terms of SubStep3 (calculate_qminus, src/SourceEuler.cpp:931-950; ideal EOS only) */
    int32_t cooling_surface; /* SurfaceCooling: thermal (src/SourceEuler.cpp:790-820) */
    int32_t opacity;         /* Opacity (src/opacity.cpp:10-43): FCPT_OPACITY_* (Lin :45-168, Bell :170-297, Constant, Simple) */
    double cooling_radiative_factor; /* CoolingRadiativeFactor */
    double kappa_const;              /* KappaConst (code units: L0^2 / M0) */
    double kappa_factor;             /* KappaFactor */
    double tau_factor;               /* TauFactor */
    double tau_min;                  /* TauMin */
    double density_factor;           /* DensityFactor */
    int32_t cooling_beta;            /* CoolingBetaLocal (thermal_relaxation, src/SourceEuler.cpp:632-786) */
    int32_t cooling_beta_reference;  /* CoolingBetaReference: FCPT_BETAREF_* */
    double cooling_beta_value;       /* CoolingBeta */
    double cooling_beta_ramp_up;     /* CoolingBetaRampUp (code time units) */
    /* unit system, code -> cgs (src/units.cpp:158-185), for the tabulated opacity laws */
    double temperature_cgs; /* K per code temperature unit */
    double density_cgs;     /* g/cm^3 per code volume-density unit */
    double opacity_cgs;     /* cm^2/g per code opacity unit */
    /* initial profiles: Sigma and e times 1 / (1 + exp(+-(r - point) / width)) (src/init.cpp:1063-1146,1363-1450,
     * src/util.cpp:69-93), floors re-applied */
    int32_t profile_cutoff_inner;       /* ProfileCutoffInner */
    int32_t profile_cutoff_outer;       /* ProfileCutoffOuter */
    double profile_cutoff_point_inner;  /* ProfileCutoffPointInner */
    double profile_cutoff_width_inner;  /* ProfileCutoffWidthInner */
    double profile_cutoff_point_outer;  /* ProfileCutoffPointOuter */
    double profile_cutoff_width_outer;  /* ProfileCutoffWidthOuter */
    /* monitoring that rides on the path */
    int32_t write_massflow; /* WriteMassFlow: accumulate the radial mass flux of every Transport() in FCPT_F_MASSFLOW */
    int32_t _pad5;
} fcpt_desc;

/* Row ranges of a slab, exactly the integers of src/split.cpp:56-78. */
typedef struct fcpt_split {
    int32_t nr;   /* local NRadial (overlap included) */
    int32_t imin; /* IMIN: global index of local row 0 */
    int32_t imax; /* IMAX */
    int32_t zero_no_ghost;
    int32_t one_no_ghost_vr;
    int32_t max_no_ghost;
    int32_t maxmo_no_ghost_vr;
    int32_t zero_or_active;
    int32_t max_or_active;
    int32_t radial_first_active;
    int32_t radial_active_size;
    int32_t is_first; /* CPU_Rank == 0 */
    int32_t is_last;  /* CPU_Rank == CPU_Highest */
} fcpt_split;

/* simulation clock, the state of namespace sim (src/simulation.cpp:24-31) */
typedef struct fcpt_clock {
    double time;
    double last_dt;
    uint64_t n_hydro_iter;
    uint32_t n_monitor;
    uint32_t n_snapshot;
} fcpt_clock;

typedef struct fcpt_ctx fcpt_ctx;

/* ---- host-side helpers (no GPU needed) -------------------------------- */

/* Fill a descriptor with the reference's defaults (src/parameters.cpp,
 * src/Interpret.cpp).  Always succeeds. */
int fcpt_desc_default(fcpt_desc *d);

/* SplitDomain (src/split.cpp:34-88) for slab d->rank of d->nranks. */
int fcpt_split_domain(const fcpt_desc *d, fcpt_split *out);

/* Interface radii Radii[0 .. nr_global + FCPT_GEOM_PAD] of the global grid
 * (src/init.cpp:92-145).  `radii` must hold nr_global + FCPT_GEOM_PAD + 1 doubles. */
int fcpt_radii(const fcpt_desc *d, double *radii);

/* Initial gas fields of slab d->rank (init_physics, src/init.cpp:255-343:
 * init_gas_density / init_gas_energy / init_gas_velocities / shock tube /
 * spreading ring) before the first boundary call.  With SetSigma0 the descriptor's
 * sigma0 is rescaled in place, as parameters::sigma0 is (src/init.cpp:1155).
 * Arrays are local-slab sized:
 * sigma, vazi, energy: nr*nphi; vrad: (nr+1)*nphi.  energy may be NULL for
 * isothermal runs. */
int fcpt_initial_fields(fcpt_desc *d, const double *radii, double *sigma, double *vrad,
                        double *vazi, double *energy);

const char *fcpt_last_error(void);

/* ---- the bodies as a system of their own (no GPU needed) ------------------
 * t_planetary_system (src/nbody/planetary_system.cpp) reduced to what the gas path's driver needs: up to
 * FCPT_MAX_BODIES point masses in the plane with positions and velocities, advanced under their mutual Newtonian
 * gravity by an extrapolation integrator (modified midpoint rule, sub-step counts 2 .. 16, Aitken-Neville in h^2:
 * order 16; internal sub-steps bounded by a tenth of the shortest two-body time and halved until the last column
 * is at rounding level).  Deterministic: the same state and arguments give the same bits on every rank.
 * Accuracy: the reference's circ_kepler_orbit criterion (1e-11 in position over 20 orbits in 2000 steps). */
typedef struct fcpt_nbody fcpt_nbody;
int fcpt_nbody_create(double G, fcpt_nbody **out);
int fcpt_nbody_destroy(fcpt_nbody *s);
int fcpt_nbody_count(const fcpt_nbody *s, int32_t *n);
/* init_planet's placement (planetary_system.cpp:162-217,483-575): the first body rests at the origin; the second is
 * put on the orbit with these elements about the first and both are moved about their barycentre (the heavier one
 * nearest the origin); every further body's elements are Jacobi elements about the centre of mass of the bodies
 * already there.  Angles in radians; a body with semi_major_axis 0 sits at that centre at rest. */
int fcpt_nbody_add(fcpt_nbody *s, double mass, double semi_major_axis, double eccentricity, double argument_of_pericenter,
                   double true_anomaly);
/* v += a dt with one acceleration per body (UpdatePlanetVelocitiesWithDiskForce, src/Pframeforce.cpp:275-293;
 * apply_indirect_term_on_Nbody) */
int fcpt_nbody_kick(fcpt_nbody *s, const double *ax, const double *ay, double dt);
/* integrate over dt (t_planetary_system::integrate); dt < 0 integrates backwards */
int fcpt_nbody_advance(fcpt_nbody *s, double dt);
/* Velocity change of the centre of mass of the first n_centre bodies over a trial advance of dt that leaves the
 * system unchanged: what ComputeIndirectTermNbody (src/frame_of_reference.cpp:135-165) divides by dt. */
int fcpt_nbody_centre_delta_v(const fcpt_nbody *s, int32_t n_centre, double dt, double out[2]);
/* positions and velocities relative to the centre of mass of the first n_centre bodies (move_to_hydro_frame_center) */
int fcpt_nbody_shift_to_centre(fcpt_nbody *s, int32_t n_centre);
/* rotate positions and velocities by `angle` about the origin (the frame's rotation: angle = -OmegaFrame dt) */
int fcpt_nbody_rotate(fcpt_nbody *s, double angle);
/* The full state (restart files), FCPT_NBODY_STATE doubles per body: {x, y, vx, vy, mass} and the four parts that the
 * integrator's compensated additions carry from step to step (0 for a body set from outside); with them a restored
 * system continues bit for bit.  get fills FCPT_NBODY_STATE * count doubles. */
#define FCPT_NBODY_STATE 9
int fcpt_nbody_get_state(const fcpt_nbody *s, double *state);
int fcpt_nbody_set_state(fcpt_nbody *s, int32_t n, const double *state);

/* ---- context ------------------------------------------------------------ */

/* One process per GPU (the reference: one MPI rank per slab, src/parallel.cpp:28-40): the number of HIP devices this
 * process sees (0 without a GPU; never fails) and the choice of the one the following fcpt_create uses.  Call
 * fcpt_set_device before any other GPU-touching call of the process. */
int fcpt_device_count(int32_t *n);
int fcpt_set_device(int32_t device);

/* Allocate all device state for slab d->rank on the current HIP device.
 * `radii` is the global interface array from fcpt_radii (or a radii.dat).
 * Replaces data.set_size + init_radialarrays + InitTransport + cfl::init
 * (src/main.cpp:96-103, src/TransportEuler.cpp:57-96, src/cfl.cpp:14-18). */
int fcpt_create(const fcpt_desc *d, const double *radii, fcpt_ctx **out);
int fcpt_destroy(fcpt_ctx *ctx);

/* Launch all subsequent work of this context on `hip_stream` (a hipStream_t;
 * NULL = the default stream).  Lets the caller order kernels against its own
 * copies / RCCL calls without extra synchronisation. */
int fcpt_set_stream(fcpt_ctx *ctx, void *hip_stream);
int fcpt_synchronize(fcpt_ctx *ctx);

/* Kernel-selection switches of one context, by name (lower case, e.g. "transport_fallback"): which of the
 * parity-tested kernel variants the step uses, marching-chunk lengths, overlap of the ghost exchange.  The
 * environment variables FCPT_<NAME> only provide the defaults read once in fcpt_create; no launch reads the
 * environment.  -1 = the library's built-in choice.  Names: transport_fused (0 = off, any other value = the built-in choice), transport_rows, transport_graded, transport_big, transport_ladder, transport_rank_grade, source_graded,
 * source_rows, theta_rows, transport_fallback, transport_split, march_source (0 = the three out-of-place source
 * kernels instead of the marching one), march_source_adi (the same for the ideal EOS only),
 * theta_march, cfl_rings, cfl_wide_blocks (-1 = built-in: isothermal 512 threads per ring, ideal EOS 256; 0 = 256; any other value = 512),
 * cfl_fold_in_source, gate_in_boundary, cfl_split, source_ring_parts, fused_damping, inline_potential, bc_fold, bc_in_cfl, comm_overlap,
 * comm_loopback, graph_steps, profile_stride (fcpt_profile_start times every n-th launch of the selected kernels).
 * fcpt_get_option also answers three read-only counters of fcpt_run_steps: graph_replays (hipGraphLaunch calls issued
 * so far), graph_cycle (steps per replay, 0 = no graph), coop_active (always 0: a one-kernel step was measured slower than
 * the launches it would replace), and transport_fell_back (1: the last Transport() met a ring pair
 * beyond the fused kernel's one-lane shift and took the two-kernel path; blocks).
 * FCPT_EINVAL for an unknown name.  (The reference has no counterpart: its variants are compile-time.) */
int fcpt_set_option(fcpt_ctx *ctx, const char *name, int32_t value);
int fcpt_get_option(const fcpt_ctx *ctx, const char *name, int32_t *value);

/* The chunks of rings into which the fused Transport() kernel (src/TransportEuler.cpp:112-136 as one marching pass)
 * divides the slab: one wavefront marches one tile of 53 cells over one chunk.  Where the slab needs several rounds of
 * the GPU's wavefront slots the library grades the chunk lengths (long chunks first: options transport_graded,
 * transport_big, transport_ladder), where one round covers it the lengths follow the rate at which a SIMD serves its
 * wavefronts (transport_rank_grade), so that the slots run dry together.  The chunking never changes a result -- every
 * ring of a tile is computed by exactly one wavefront from the same operands.
 * fcpt_transport_chunks reports (tile, first ring, one past the last ring) per wavefront in the order of dispatch, entries
 * with first == last being idle (n_wavefronts = 0: equal chunks of transport_rows rings); fcpt_set_transport_chunks
 * replaces the lengths by an explicit list of chunk lengths, dealt from both ends of the slab, the last entry repeating
 * (n = 0: back to the built-in choice) -- a tuning and test hook, like the options.
 * (No counterpart in the reference: its loops are not chunked.) */
int fcpt_set_transport_chunks(fcpt_ctx *ctx, const int32_t *lengths, int32_t n);
int fcpt_transport_chunks(const fcpt_ctx *ctx, int32_t *tile_first_last, int32_t capacity, int32_t *n_wavefronts);
/* Likewise the marching kernels of the source step (update_with_sourceterms ... SubStep3 as one pass, src/SourceEuler.cpp,
 * src/viscosity/): where one round of wavefronts covers the slab, every wavefront's chunk length is matched to the rate at
 * which its SIMD will serve it (option source_graded, per cent of difference between first and last rank; 0: equal
 * chunks).  Reports (segment of 59 cells, first ring, one past the last ring) per wavefront in the order of dispatch,
 * entries with first == last being idle; n_wavefronts = 0: equal chunks of source_rows rings.
 * fcpt_set_source_chunks replaces the table by one cut from an explicit list of chunk lengths -- a tuning and test hook,
 * like the options: the rows 0 .. nr of v_r are cut from row 0 upward, the last entry repeating, a remainder of fewer than
 * 3 rings joined to the chunk before it, the same cut for every segment; entries chunk by chunk, the segments of a chunk
 * side by side, padded with idle entries to whole workgroups of 4 wavefronts (n = 0: back to the built-in choice).  The
 * list stays in force across fcpt_set_option; source_rows > 0 selects equal chunks over it, source_graded does not matter
 * to it.  FCPT_EINVAL for a length below 3 (a table's edge chunks apply the pre-transport boundary call, which reads three
 * rows they must have stored themselves), for more wavefronts than the table holds (16 448), and between fcpt_step and
 * fcpt_post.  The chunking never changes a result. */
int fcpt_set_source_chunks(fcpt_ctx *ctx, const int32_t *lengths, int32_t n);
int fcpt_source_chunks(const fcpt_ctx *ctx, int32_t *seg_first_last, int32_t capacity, int32_t *n_wavefronts);

int fcpt_get_split(const fcpt_ctx *ctx, fcpt_split *out);
int fcpt_get_clock(const fcpt_ctx *ctx, fcpt_clock *out);
int fcpt_set_clock(fcpt_ctx *ctx, const fcpt_clock *in);
/* hydro_dt_logger (src/hydro_dt_logger.h:13-34: "min dt" / "max dt" of monitor/timestepLogging.dat): the smallest and
 * largest step length since the last call with reset != 0, kept next to the device clock so that callers who let
 * fcpt_run_steps run many steps without reading dt still get them.  Blocks. */
int fcpt_dt_statistics(fcpt_ctx *ctx, double *dt_min, double *dt_max, int32_t reset);

/* Host <-> device copies of one grid in the reference's Field layout
 * (what read2D / write2D move, src/polargrid.cpp:135-180,301-353).
 * Synchronous with respect to the context's stream. */
int fcpt_upload(fcpt_ctx *ctx, int32_t field, const double *host);
int fcpt_download(fcpt_ctx *ctx, int32_t field, double *host);
/* Device address and element count of a grid, for zero-copy callers.  The transport is out of place:
 * the addresses of SIGMA, ENERGY, VRAD and VAZI may change in fcpt_step / fcpt_step_device /
 * fcpt_run_steps -- query again after a step. */
int fcpt_device_ptr(fcpt_ctx *ctx, int32_t field, void **dptr, uint64_t *count);

/* Positions, masses and cubic smoothing radii of the N-body objects for the
 * next potential evaluation, plus the indirect-term acceleration
 * (CalculateNbodyPotential, src/Pframeforce.cpp:21-94).  Body 0 is the star. */
int fcpt_set_bodies(fcpt_ctx *ctx, int32_t n, const double *x, const double *y, const double *mass,
                    const double *cubic_smoothing_radius, double indirect_x, double indirect_y);

/* Leapfrog only: the bodies at the mid-step time, used for the potential of the second gas
 * kick (src/simulation.cpp:359-366).  Without this call the second kick reuses the positions of
 * fcpt_set_bodies.  Must follow fcpt_set_bodies (same n). */
int fcpt_set_bodies_midstep(fcpt_ctx *ctx, int32_t n, const double *x, const double *y, const double *mass,
                            const double *cubic_smoothing_radius);

/* Stellar irradiation of the disk in SubStep3 (irradiation_single, src/SourceEuler.cpp:538-612): body k
 * of fcpt_set_bodies heats the gas if temperature[k] > 0 (code units), with its radius (code units)
 * and the ramp-up time of the heating.  Any irradiating body also switches the effective optical
 * depth to the irradiated form (kappa_eff, src/compute.cpp:64-77).  Ideal EOS only. */
int fcpt_set_body_irradiation(fcpt_ctx *ctx, int32_t n, const double *temperature, const double *radius,
                              const double *rampup_time);

/* Specific force of this slab's gas on an object at (x, y): ComputeDiskOnPlanetAccel
 * (src/Force.cpp:23-122) without its MPI_Allreduce -- out = {a_x, a_y} summed over the cells
 * of the rings inside `r_object` (the object's distance to the origin) followed by {a_x, a_y}
 * of the rings outside, over this slab's active rings; the caller adds the slabs' four sums
 * (the reference's 4-double all-reduce) and then inner + outer.  Smoothing as
 * compute_smoothing (src/Force.cpp:124-159): `smoothing_fixed` < 0 selects
 * ThicknessSmoothing x H of each cell, a value >= 0 is used as it is (planet-location smoothing,
 * or 0 for the star with compatibility_no_star_smoothing).  `cubic_smoothing_radius` > 0 applies
 * the derivative of the Klahr & Kley cubic smoothing inside that distance.
 * Blocks until the four sums are on the host. */
int fcpt_disk_on_body_accel(fcpt_ctx *ctx, double x, double y, double r_object, double smoothing_fixed,
                            double cubic_smoothing_radius, double out[4]);

/* The same four sums for n <= FCPT_MAX_BODIES objects from ONE pass over the slab's active rings (the density, and
 * the energy or scale-height grid where a body asks for cell-wise smoothing, are read once for all bodies); body k is
 * defined by (x[k], y[k], r_object[k], smoothing_fixed[k], cubic_smoothing_radius[k]) exactly as in the single-body
 * call, whose kernel is mirrored cell by cell and sum by sum: out[4k .. 4k+3] carries the bits that call returns.
 * _begin queues the pass and an asynchronous copy of the 4n sums into pinned host memory on the context's stream and
 * returns; _end waits for that copy alone (an event) and hands out the sums of this slab.  A host-stepped loop queues
 * _begin in front of fcpt_cfl, whose wait then covers both.  FCPT_EINVAL: n outside 1 .. FCPT_MAX_BODIES, _end
 * without a pending _begin.  The caller adds the slabs' sums with fcpt_allreduce_sum. */
int fcpt_disk_on_bodies_begin(fcpt_ctx *ctx, int32_t n, const double *x, const double *y, const double *r_object,
                              const double *smoothing_fixed, const double *cubic_smoothing_radius);
int fcpt_disk_on_bodies_end(fcpt_ctx *ctx, double *out /* 4n */);

/* After the initial Sigma/v/energy upload: init_euler (src/SourceEuler.cpp:251-285:
 * sound speed, pressure, temperature, scale height, viscosity), the first
 * potential, copy_initial_values + apply_boundary_condition + copy_initial_values
 * (src/init.cpp:337-341). */
int fcpt_init_physics(fcpt_ctx *ctx);

/* recalculate_derived_disk_quantities (src/SourceEuler.cpp:225-249) after the state grids were replaced from
 * outside (restart_load, src/restart.cpp:18-139: uploads of Sigma, vrad, vazi, energy, Qplus, Qminus and of the
 * t = 0 grids into FCPT_F_*0, then this call). */
int fcpt_recalculate_derived(fcpt_ctx *ctx);

/* ---- Lagrangian dust particles with gas drag and diffusion ---------------------------------------------------------------
 * particles::integrate with ParticleIntegrator: midpoint (integrate_exponential_midpoint, src/particles/
 * particles.cpp:1579-1672, after Zhu et al. 2014 and Mignone et al. 2019) on one radial slab (on several: see
 * fcpt_particles_slabs, below), for the host-stepped
 * loop: per step fcpt_set_bodies, fcpt_particles_step, fcpt_step, fcpt_post -- the particle step reads the gas at the
 * start of the hydro step, where the reference calls it (src/simulation.cpp:177-180).  fcpt_run_steps advances
 * particles only after fcpt_particles_follow_run_steps(ctx, 1), below.  A context that never receives particles launches
 * nothing for them.
 *
 * Departure from the reference: a particle beyond Rmed[Nr-1] makes the reference read row Nr of a scalar grid (out
 * of bounds); here the lower row of the cell-centred interpolation is clamped to [0, Nr-2] (linear extrapolation
 * from the last two rows, the mirror of the release build's behaviour below Rmed[0]) and that of v_r to [0, Nr-1].
 * ParticleIntegrator: explicit (integrate_explicit_adaptive, :1677-2014) with its CartesianParticles state is selected
 * with fcpt_particles_integrator, below; the host driver does not offer it yet and still refuses the key.
 * Not covered (the host driver refuses setups that ask for them): disk gravity on particles, leapfrog, particles on
 * several slabs in the host driver (the library runs them, inside fcpt_run_steps too: fcpt_particles_slabs, below). */
typedef struct fcpt_particle_params {
    double particle_density;  /* ParticleDensity (code units) */
    double molecule_mass;     /* mu * m_u (code units), calc_tstop's m0 (particles.cpp:1139) */
    double molecule_radius;   /* 1.5e-8 cm in code units (particles.cpp:1147) */
    double k_B;               /* Boltzmann's constant (code units) */
    double escape_radius_min; /* ParticleMinimumEscapeRadius, inside [rmin, rmax] of the descriptor */
    double escape_radius_max; /* ParticleMaximumEscapeRadius */
    int32_t gravity_cartesian; /* 1: the bodies' pull in Cartesian form (particles.cpp:1020-1060: CartesianParticles: yes
                                * with the midpoint integrator, parameters.cpp:927-932), 0: polar form (:981-1018) */
    int32_t _pad0;
} fcpt_particle_params;

/* The values of the default unit system (L0 = 1 au, M0 = 1 solMass; fcpt_desc_default) for d->mu, escape radii at
 * d->rmin / d->rmax, polar gravity.  No GPU needed. */
int fcpt_particle_params_default(const fcpt_desc *d, fcpt_particle_params *out);

/* Replace the particles of the context by n particles (host arrays of n entries each, copied; the caller's order is
 * kept: slot k holds particle k).  r, phi: position; r_dot, phi_dot: dr/dt and dphi/dt; radius: grain radius;
 * stokes: the Stokes number of the previous step (enters the smoothing length, particles.cpp:896-912; check_tstop's
 * value at the start).  n = 0 removes them.  FCPT_EINVAL: a context that is one of several slabs and has not opted in
 * with fcpt_particles_slabs, escape radii outside [rmin, rmax] or not ordered, a null array.  Blocks. */
int fcpt_particles_set(fcpt_ctx *ctx, const fcpt_particle_params *params, int64_t n, const uint64_t *id, const double *r,
                       const double *phi, const double *r_dot, const double *phi_dot, const double *radius,
                       const double *stokes);

/* One launch on the context's stream, no host wait: update_velocities_from_indirect_term (particles.cpp:1326-1341)
 * with (indirect_x, indirect_y), integrate_exponential_midpoint over dt with the gas grids as they are and the bodies
 * of the last fcpt_set_bodies (star included), the escape test of move() (:2019-2031: a particle with r^2 beyond the
 * squared escape radii -/+ DBL_EPSILON is dead from then on) and rotate (:2394-2395) by frame_angle (= OmegaFrame dt).
 * Where the reference's calc_tstop would die() (Ma, CdE, CdS, Cd outside their ranges, :1163-1208) nothing of the
 * particle is written in that step -- neither the indirect term's kick nor the rotation by frame_angle, so in a rotating
 * frame it stays behind its neighbours -- and its id and the guard (1 .. 8 in the order of the source) are kept for the
 * next blocking call.  If several particles trip a guard between two blocking calls, any one of them is the one
 * reported (plain stores of the lanes to one status word: which one is not deterministic).
 * In the column search an angle whose product with Nphi / 2 pi rounds up to Nphi stays in the last column (the reference
 * wraps it to column 0 and extrapolates v_phi over a whole turn there). */
int fcpt_particles_step(fcpt_ctx *ctx, double dt, double indirect_x, double indirect_y, double frame_angle);

/* Block until the queued particle steps are done.  _count: the number of live particles.  _get: the live particles in
 * ascending slot order (arrays of `capacity` entries, any of them may be NULL; FCPT_EINVAL if capacity is too small,
 * *n then tells the need).  Both return FCPT_EINVAL once when a guard was tripped since the last blocking call
 * (fcpt_last_error names the particle's id and the guard), and work again afterwards. */
int fcpt_particles_count(fcpt_ctx *ctx, int64_t *n_alive);
int fcpt_particles_get(fcpt_ctx *ctx, int64_t capacity, uint64_t *id, double *r, double *phi, double *r_dot, double *phi_dot,
                       double *radius, double *stokes, int64_t *n);

/* Turbulent diffusion of the dust as a random walk (ParticleDustDiffusion: yes; src/particles/dust_diffusion.cpp:29-97,
 * Charnoz et al. 2011 eq. 17) and ParticleGasDragEnabled.  With diffusion on, fcpt_particles_step ends, before the
 * escape test, with the radial kick
 *   dr = D_d / rho  d rho / dr  dt^2 Omega_K + snv sigma + r (sqrt(1 + (sigma snv / r)^2) - 1),  sigma = sqrt(2 D_d dt),
 *   D_d = alpha c_s H / Sc,  Sc = (1 + St^2)^2 / (1 + 4 St^2),  phi_dot *= (r_old / r_new)^1.5
 * from the values of the particle's cell (row of get_rinf_id, no interpolation; d rho / dr is the central difference
 * over Rmed and zero in rows 0 and Nr-1; alpha is ViscousAlpha whatever the viscosity law).  A kicked radius <= 0
 * counts as escaped.
 * snv is a standard normal deviate that depends only on (seed, particle id, step): Philox4x32-10 with
 *   counter = (id low, id high, step low, step high), key = (seed low, seed high),
 *   u1 = ((w0 << 20 | w1 >> 12) + 0.5) 2^-52, u2 likewise from (w2, w3), snv = sqrt(-2 log u1) cos(2 pi u2),
 * so the result does not depend on the slot order or on where a run was restarted.  `step` is advanced by one by every
 * fcpt_particles_step, whatever the switches and also when there are no particles.  Ids must be distinct while
 * diffusion is on: fcpt_particles_diffusion and fcpt_particles_set return FCPT_EINVAL otherwise.
 * With gas_drag = 0 the stopping time is 1e100 and no drag term is applied (particles.cpp:1616-1656); the Stokes number
 * the step leaves is 1e100 Omega_K(r) without diffusion and, with it, that of check_tstop (:1277-1311) at the end
 * position, whose guards are reported as those of the drag step.
 * Departure from the reference: rho, d rho / dr and D_g are formed from the current Sigma (and e); the reference
 * evaluates them at init and refreshes them only under Disk: yes (from a RHO that follows the gas only with the drag
 * on).  The two agree for frozen gas.
 * The settings belong to the context and outlive fcpt_particles_set.  A context that never calls
 * fcpt_particles_diffusion steps with {1, 0, 0, 0}. */
typedef struct fcpt_particle_diffusion {
    int32_t gas_drag;  /* 1 (default) | 0: ParticleGasDragEnabled */
    int32_t diffusion; /* 0 (default) | 1: ParticleDustDiffusion */
    uint64_t seed;     /* Philox key */
    uint64_t step;     /* Philox counter of the next fcpt_particles_step */
} fcpt_particle_diffusion;
int fcpt_particles_diffusion(fcpt_ctx *ctx, const fcpt_particle_diffusion *p);
int fcpt_particles_diffusion_get(fcpt_ctx *ctx, fcpt_particle_diffusion *out); /* with the current step */
/* The deviates the live particles would draw at counter `step` with the context's seed, in fcpt_particles_get's order
 * (one small launch; nothing is stepped).  capacity as for fcpt_particles_get. */
int fcpt_particles_normals(fcpt_ctx *ctx, uint64_t step, int64_t capacity, double *snv);

/* ParticleIntegrator: explicit (integrate_explicit_adaptive, particles.cpp:1677-2014), the integrator for weakly coupled
 * bodies (t_stop >= 10 dt).  With kind = 1 fcpt_particles_step queues, in one launch and per live particle:
 * update_velocities_from_indirect_term (:1314-1343; the Cartesian form :1322-1324 with cartesian = 1); with gas_drag the
 * explicit kick of update_velocities_from_gas_drag(_cart) (:1428-1504, :1345-1418: skipped for r < RMIN or r > RMAX, else
 * v += dt a_drag and stokes = t_stop Omega_K(r), the gas interpolated as for the midpoint step with the same
 * out-of-range departures); the embedded Cash-Karp RK5(4) over dt in substeps of the particle's own `timestep`
 * (atol 1e-14, rtol 1e-12, Lund-stabilised controller, :1693-2012), the smoothing length recomputed every substep from
 * the cell of the current position (:896-912) and the pull of the bodies of the last fcpt_set_bodies with the softening
 * inside the square root (:914-952, or :954-979 with cartesian = 1); the escape test of move() on the squared distance
 * (x^2 + y^2 with cartesian = 1); rotate (:2369-2397: position and velocity are turned with cartesian = 1).
 * The controller is restated as written, with the aliasing of :1726: old_timestep refers to the stored step, which
 * already holds the new value after :1981, so a rejection divides the stored step twice.
 * cartesian = 1: r, phi, r_dot, phi_dot of fcpt_particles_set / _get hold x, y, v_x, v_y (CartesianParticles: yes).
 * Guards, reported like those of calc_tstop and leaving the particle exactly as it was (timestep and facold included):
 *   9   accepted + rejected substeps of one particle in one call reached max_attempts.  The reference's loop has no
 *       bound; a NaN or zero step size would spin for ever.
 *   10  t_stop < 10 dt in the drag kick.  Departure: check_tstop (:1303-1309) exits the reference on this condition once,
 *       at start-up, and calls the explicit kick unstable below it; here it is held at every step.
 * The step sizes live in a second device allocation made by fcpt_particles_timestep_init (queues
 * init_particle_timestep, :248-374: Hairer's starting step with rsmooth = 0.05, facold = 1e-4) or
 * fcpt_particles_adaptive_set (restart: n = the number of slots of the last fcpt_particles_set, slot order).
 * fcpt_particles_set invalidates them: fcpt_particles_step with kind = 1 returns FCPT_EINVAL until one of the two has
 * run.  fcpt_particles_adaptive_get blocks and hands out, for the live particles in slot order (any array may be NULL),
 * the step size, facold, the accelerations of the last accepted substep and the accepted / rejected substeps of the last
 * call.
 * FCPT_EINVAL: kind = 1 while diffusion is on, and diffusion = 1 while kind = 1 (whichever call comes second; the
 * refused call changes nothing); cartesian = 1 with kind = 0 (the midpoint integrator's Cartesian gravity remains
 * fcpt_particle_params.gravity_cartesian); max_attempts < 0.
 * The settings belong to the context and outlive fcpt_particles_set.  A context that never selects kind = 1 allocates
 * and launches what it did before. */
typedef struct fcpt_particle_integrator {
    int32_t kind;         /* 0 midpoint (default) | 1 explicit adaptive */
    int32_t cartesian;    /* explicit only: r, phi, r_dot, phi_dot hold x, y, vx, vy (CartesianParticles) */
    int32_t max_attempts; /* explicit only; 0 = 10000 */
    int32_t _pad0;
} fcpt_particle_integrator;
int fcpt_particles_integrator(fcpt_ctx *ctx, const fcpt_particle_integrator *p);
int fcpt_particles_integrator_get(fcpt_ctx *ctx, fcpt_particle_integrator *out);
int fcpt_particles_timestep_init(fcpt_ctx *ctx);
int fcpt_particles_adaptive_set(fcpt_ctx *ctx, int64_t n, const double *timestep, const double *facold);
int fcpt_particles_adaptive_get(fcpt_ctx *ctx, int64_t capacity, double *timestep, double *facold, double *r_ddot,
                                double *phi_ddot, uint32_t *accepted, uint32_t *rejected, int64_t *n);

/* Particles inside fcpt_run_steps.  on = 1: every iteration of fcpt_run_steps also takes the particle step (on one of
 * several slabs: and the migration, see "Inside fcpt_run_steps" under fcpt_particles_slabs, below), where the reference
 * has it (src/simulation.cpp:177-180): after the step length of the iteration is in force and
 * before the gas step, so it reads the gas of the start of the hydro step.  It is the step fcpt_particles_step would
 * take with dt = the step length the gas step uses, (indirect_x, indirect_y) and the bodies of the last fcpt_set_bodies
 * and frame_angle = OmegaFrame dt (one rounded product), with the integrator, cartesian, gas_drag and diffusion settings
 * of the context, and it advances the Philox counter by one.  With snap != 0 fcpt_run_steps calls fcpt_particles_step
 * itself; with snap = 0 the kernels take dt, frame_angle and the counter from device memory, nothing comes to the host,
 * and the launch is part of the hipGraph replayed on launch-bound grids (the CFL fold inside the marching source kernel
 * gives way to the policy launch while particles are present; the gas bits are the same).  A captured graph is replayed
 * only while the particle launch it holds is the one the context would queue now: whatever fcpt_particles_set,
 * _diffusion, _integrator, _adaptive_set, _timestep_init, fcpt_set_bodies or this call change in it leads to a new
 * capture, never to a stale replay (a setting put back before the next fcpt_run_steps changes nothing).  When
 * fcpt_run_steps returns, fcpt_particles_diffusion_get().step has advanced by *nsteps_done, also when there are no
 * particles.  Guards 1 .. 10 go to the status word and are reported once by the next blocking particle call, as after
 * fcpt_particles_step.  Bodies do not move inside fcpt_run_steps.
 * fcpt_run_steps returns FCPT_EINVAL, with *nsteps_done = 0, the clock untouched and nothing queued, while this is on and
 * the descriptor selects Integrator: Leapfrog, or the explicit integrator is selected and has no step sizes since the
 * last fcpt_particles_set, or the context is one of several slabs and lacks a communicator or fcpt_particles_slabs
 * {on = 1} (the message names which).
 * The setting belongs to the context and outlives fcpt_particles_set.  The default is 0: a context that never switches it
 * on allocates, launches and computes what it did before. */
int fcpt_particles_follow_run_steps(fcpt_ctx *ctx, int32_t on);
int fcpt_particles_follow_run_steps_get(const fcpt_ctx *ctx, int32_t *on);

/* ---- particles on several radial slabs: ownership and migration (particles::move, src/particles/particles.cpp:2016-2161)
 * Opt-in with fcpt_particles_slabs {on = 1}; without it fcpt_particles_set on one of several slabs is refused as before.
 *
 * Ownership.  Every slab is handed the SAME full list by fcpt_particles_set and holds all n slots (slot k is particle k
 * on every slab, about 57 bytes per particle and slab), but steps only the particles it owns: alive[k] is set where
 * r_lo^2 <= d^2 < r_hi^2, d^2 = r^2 (x^2 + y^2 with cartesian = 1) and [r_lo, r_hi] the window of
 * fcpt_particles_slab_window: Rinf of local row FCPT_OVERLAP and of local row nr - FCPT_OVERLAP (local_r_min /
 * local_r_max of particles.cpp:527-529), -inf on the first and +inf on the last slab (at the grid's own edges the escape
 * radii act first).  Neighbouring slabs return the same bits at their shared edge.  Needs no GPU.
 *
 * Migration.  After fcpt_particles_step a live owned particle with d^2 < r_lo^2 goes to the inner neighbour, one with
 * d^2 > r_hi^2 to the outer one (:2067, :2126; exactly on an edge it stays): its alive byte is cleared by the sender and
 * set by the receiver.  A record is the slot index followed by r, phi, r_dot, phi_dot, stokes and, once the explicit
 * integrator's step sizes exist (they must then exist on every slab), timestep, facold, r_ddot, phi_ddot: R = 6 or 10
 * doubles; id and radius are replicated and do not travel, the substep counters of fcpt_particles_adaptive_get stay with
 * the slab that took the step.  A migration message of the calls below is always exactly fcpt_exchange_count doubles
 * long (inside fcpt_run_steps it is cut to what the capacity can fill, see there): word 0 holds the record count (as a
 * double), the records follow, the rest is unspecified -- so the communicator of the ghost rings carries it unchanged.
 * migrate_capacity records per side and call; 0 selects the built-in (fcpt_exchange_count - 1) / R, a larger value is
 * FCPT_EINVAL (when given, and again when the records grow to 10 doubles: the capacity in force is the smaller).  The
 * leavers of a side are served in ascending slot order, and the records stand in the message in that order.  A particle
 * beyond the capacity stays with its owner, alive, and is counted in `deferred`: the overlap rings still hold its gas,
 * and the next call takes it.  Who goes and who waits depends on the particles alone, so two runs of one state agree
 * in every message, counter and bit.
 *   fcpt_particles_migrate_pack / _unpack / _count mirror fcpt_exchange_pack / _unpack / _count (host or device buffers
 *   of _count doubles, NULL skips a side): slabs of one process hand the messages over themselves.  _unpack reads the
 *   count on the device and scatters by slot index; a record whose slot index is not in 0 .. n-1, or a count beyond the
 *   capacity, writes nothing and is reported by the next blocking particle call ("guard 12").
 *   fcpt_particles_migrate is the collective: pack, the neighbour exchange of the context's communicator on the
 *   context's stream, unpack (blocks with the host link, stream-ordered with RCCL).  FCPT_EINVAL without a communicator
 *   or without on.
 * The per-slot state is a function of the inputs alone, so the slabs' states merged by slot carry the bits of a one-slab
 * run on the same gas.  fcpt_particles_get / _count / _adaptive_get / _normals return the owned live particles in
 * ascending slot order; the caller merges the slabs and sums counts (fcpt_allreduce_sum).
 *
 * Guard 11.  On a slab the step reports a particle that needs a gas row beyond the slab's rings on a side that has a
 * neighbour (it moved more than the overlap in one step, or was deferred too long), where a one-slab run would read
 * real gas and the clamps of the cell search would extrapolate silently: the lower row of a cell-centred interpolation
 * or of the smoothing cell is below 0 or above nr - 3 (v_r is read up to two rows above it, and its row nr is not part
 * of the ghost exchange), or the row of the diffusion kick is below 1 or above nr - 2.  As with guards 1 .. 10 nothing of
 * the particle is written and the id and the guard come back at the next blocking call.  The clamps at the grid's own
 * inner and outer edge are unchanged.
 *
 * Inside fcpt_run_steps (fcpt_particles_follow_run_steps on, nranks > 1).  The context needs a communicator
 * (fcpt_comm_init or fcpt_comm_init_host) and on = 1; without either fcpt_run_steps returns FCPT_EINVAL before anything
 * is queued (*nsteps_done = 0, the clock untouched), and the message of the multi-slab refusal names what is missing.
 * Every slab's host calls fcpt_run_steps with the same arguments.  The order of an iteration:
 *   snap = 0 (dt never leaves the device): CFL reduction and MIN all-reduce, time-step policy kernel, particle step (the
 *     slab kernels in their clock-reading form: dt, OmegaFrame dt and the Philox counter come from device memory),
 *     migration (pack, neighbour exchange on the context's stream, unpack), gas step, ghost exchange, post;
 *   snap != 0: all-reduced CFL value to the host, fcpt_calculate_timestep, fcpt_snap_to_monitor, fcpt_particles_step(dt,
 *     the indirect term of the last fcpt_set_bodies, OmegaFrame dt), fcpt_particles_migrate, fcpt_step, fcpt_exchange,
 *     fcpt_post.
 * Both give the bits of the same sequence called from the host.  The collective is issued in every iteration while follow
 * and on are set, also on a context without particles (empty messages, no particle kernel), so that every slab makes the
 * same calls.  With snap = 0 a migration message carries 1 + C R doubles, C the capacity in force (equal on all slabs, like
 * R): a small migrate_capacity moves a small message every step.  fcpt_particles_migrate and _pack / _unpack / _count
 * keep the full length.  The four totals below and fcpt_particles_diffusion_get().step keep running; guards 1 .. 12 are
 * reported by the next blocking particle call.  No hipGraph is captured for a context with a communicator.
 * The host driver does not run particles with --ranks.
 * sent_inner, sent_outer, received, deferred are running totals since fcpt_create, read-only (fcpt_particles_slabs
 * ignores them); fcpt_particles_slabs_get blocks.  The setting belongs to the context and outlives fcpt_particles_set;
 * switch it before fcpt_particles_set. */
typedef struct fcpt_particle_slabs {
    int32_t on;               /* 1: this context takes particles as one of several slabs */
    int32_t migrate_capacity; /* records per side and call, 0: built-in */
    uint64_t sent_inner, sent_outer, received, deferred;
} fcpt_particle_slabs;
int fcpt_particles_slab_window(const fcpt_desc *d, const double *radii, double window[2]);
int fcpt_particles_slabs(fcpt_ctx *ctx, const fcpt_particle_slabs *p);
int fcpt_particles_slabs_get(fcpt_ctx *ctx, fcpt_particle_slabs *out);
int fcpt_particles_migrate_count(fcpt_ctx *ctx, uint64_t *count);
int fcpt_particles_migrate_pack(fcpt_ctx *ctx, double *send_inner, double *send_outer);
int fcpt_particles_migrate_unpack(fcpt_ctx *ctx, const double *recv_inner, const double *recv_outer);
int fcpt_particles_migrate(fcpt_ctx *ctx);

/* The generator itself, on the host (no GPU needed): ten rounds of Philox4x32, and the deviate above. */
void fcpt_philox4x32(const uint32_t ctr[4], const uint32_t key[2], uint32_t out[4]);
double fcpt_particles_std_normal(uint64_t seed, uint64_t id, uint64_t step);

/* ---- self-gravity of the gas ------------------------------------------------------------------------------------------
 * selfgravity::compute (src/selfgravity.cpp:303-319) in the modes SelfGravityMode: basic (sg_B) and symmetric (sg_S): the
 * polar convolution of Baruteau (2008) on a logarithmic grid.  The reduced densities S_r = Sigma sqrt(Rmed / Rmed[0]) and
 * S_t = S_r Rmed / Rmed[0] are laid into the lower Nr rows of a zero-padded array of 2 Nr rows (:321-416), transformed,
 * multiplied with the spectra of the kernel tables K_radial / K_azimuthal (:418-518, built on the host with libm from Radii[]
 * and epsilon = thickness_smoothing_sg * aspect_ratio, or lambda_sq and chi_sq of :171-179) and with -G, transformed back
 * and weighted ring by ring with r_step t_step / (2 Nr Nphi) and the powers of Rmed / Rmed[0] (:520-703).  The results are
 * the grids FCPT_F_SG_ACCEL_RAD / _AZI.  The kick is update_velocities (:712-747): v_r rows 1 .. Nr-1 from g_r of rows i and
 * i-1, v_phi rows 0 .. Nr-1 from g_phi of columns j and j-1 (wrapping); v_r rows 0 and Nr stay untouched.
 *
 * The transforms are the library's own (csrc/kernels/fft.h: a mixed-radix Stockham transform in LDS, radices 2, 3, 4, 5, one
 * row per workgroup); no FFT library is linked.  Both real fields ride in one complex transform and are separated by
 * Hermitian symmetry in the multiply.
 * Departures from the reference: (1) FFTW takes any length; here Nphi and 2 Nr must each be at most 8192 and have no
 * prime factor above 5, anything else is refused with FCPT_EINVAL and the length named.  (2) One slab only: a context that is
 * one of several slabs is refused.  (3) SelfGravityMode: besselkernel, which rescales the scale height by Toomre's Q
 * inside the source step, is not built.  (4) The caller supplies the aspect ratio h of the kernel; the reference's refresh
 * from the mass-averaged aspect ratio every 20 steps under the ideal EOS (:186-214) is the caller's: call fcpt_selfgravity
 * again.  The result agrees with the reference's to rounding, not to the bit (another transform, another order of sums).
 *
 * Memory: 96 bytes per cell for the transforms and spectra plus the two grids, allocated by fcpt_selfgravity and freed by
 * mode 0 or fcpt_destroy; a context that never calls fcpt_selfgravity allocates, launches and computes what it did before.
 * in_step = 1: every gas kick of fcpt_step / fcpt_step_device / fcpt_run_steps begins with compute + kick over the kick's own
 * step length (update_with_sourceterms, src/SourceEuler.cpp:435-441; Leapfrog: both half kicks with dt / 2,
 * src/simulation.cpp:324, 379), read from the device clock: no host round trip, serial launches on the context's stream, also
 * inside the captured graph of fcpt_run_steps.  The step length must be final before the kick, so with in_step the CFL fold
 * inside the marching source kernel gives way to the policy launch (the gas bits are the same).
 * fcpt_selfgravity returns FCPT_EINVAL, fcpt_last_error naming the reason, for: a grid that is not logarithmic
 * (selfgravity.cpp:222), a context that is one of several slabs, a refused length, aspect_ratio <= 0, an unknown mode.  A
 * refused call changes nothing.  Blocks (it builds, uploads and transforms the kernel tables). */
#define FCPT_FFT_MAX_N 8192 /* the longest transform: Nphi and 2 Nr of a self-gravitating grid */
enum { FCPT_SG_OFF = 0, FCPT_SG_BASIC = 1, FCPT_SG_SYMMETRIC = 2 };
typedef struct fcpt_selfgravity_params {
    int32_t mode;     /* 0 off, FCPT_SG_BASIC 1, FCPT_SG_SYMMETRIC 2 */
    int32_t in_step;  /* 1: every kick of fcpt_step / _step_device / _run_steps begins with the SG kick */
    double aspect_ratio, thickness_smoothing_sg;
} fcpt_selfgravity_params;
int fcpt_selfgravity(fcpt_ctx *ctx, const fcpt_selfgravity_params *p); /* (re)builds the kernel spectra; mode 0 frees */
int fcpt_selfgravity_get(fcpt_ctx *ctx, fcpt_selfgravity_params *out);
/* compute(data, 0, false): fills the two grids from the current density; asynchronous, no host wait */
int fcpt_selfgravity_compute(fcpt_ctx *ctx);
/* compute(data, dt, true): compute + update_velocities; asynchronous */
int fcpt_selfgravity_kick(fcpt_ctx *ctx, double dt);
/* Test hooks.  _kernel (no GPU needed): the tables K_radial and K_azimuthal fcpt_selfgravity would upload for this descriptor,
 * these global radii and parameters, 2 Nrad x Nphi doubles each, row-major (capacity: doubles per array).  _fft_radices (no
 * GPU needed): the radices of the stages of a transform of length n, in the order they run; FCPT_EINVAL for a refused length.
 * _fft: `rows` rows of n interleaved complex numbers (re, im) transformed in place on the device with exp(-2 pi i jk / n)
 * (inverse != 0: exp(+2 pi i jk / n)), unnormalised; blocks. */
int fcpt_selftest_selfgravity_kernel(const fcpt_desc *d, const double *radii, const fcpt_selfgravity_params *p,
                                     double *k_radial, double *k_azimuthal, int64_t capacity);
int fcpt_selftest_fft_radices(int32_t n, int32_t *radices, int32_t capacity, int32_t *count);
int fcpt_selftest_fft(int32_t rows, int32_t n, int32_t inverse, double *interleaved);

/* ---- the hot path -------------------------------------------------------- */

/* cfl::condition_cfl without the MPI_Allreduce (src/cfl.cpp:185-376): the
 * minimum over this slab's active rings.  Blocks until the value is on the host. */
int fcpt_cfl(fcpt_ctx *ctx, double *dt_local);

/* Device-resident variants for multi-slab runs that keep dt off the host: fcpt_cfl_device
 * writes this slab's CFL minimum to *d_dt_local (a device address, e.g. of a tensor the
 * caller then MIN-all-reduces with RCCL on the same stream); fcpt_calculate_timestep_device
 * applies the CalculateTimeStep policy to the reduced value read from *d_cfl_global (NULL: the value
 * fcpt_cfl_allreduce left in the library's own device scalar) and
 * leaves the step length in the device clock, where fcpt_step_device / fcpt_post_device
 * pick it up.  No call in this group synchronises with the host. */
int fcpt_cfl_device(fcpt_ctx *ctx, double *d_dt_local);
int fcpt_calculate_timestep_device(fcpt_ctx *ctx, const double *d_cfl_global);
int fcpt_step_device(fcpt_ctx *ctx);
int fcpt_post_device(fcpt_ctx *ctx);

/* fcpt_step_device for slabs with neighbours, in two halves around the caller's ghost exchange: _begin queues
 * the source step and marches the chunks of the transport that hold the rings the neighbours are waiting for
 * (rows [7,14) and [nr-14,nr-7)) on the context's stream and all other chunks on an internal stream; the
 * caller then queues fcpt_exchange_pack and its transfers, which run under the interior chunks; _end makes the
 * context's stream wait for them.  Between the two only fcpt_exchange_pack may be called.  Same results as
 * fcpt_step_device (the chunks are independent); falls back to it (and _end is a no-op) when the one-kernel
 * transport does not apply: leapfrog, rings shorter than 256 cells, a dt that is not the CFL policy's. */
int fcpt_step_device_begin(fcpt_ctx *ctx);
int fcpt_step_device_end(fcpt_ctx *ctx);

/* Hides the ghost exchange behind the next step's CFL reduction (slabs with neighbours): queued after
 * fcpt_step* and fcpt_exchange_pack, before the caller waits for the neighbours' rings, it evaluates
 * condition_cfl (src/cfl.cpp:222-330) on the rings that neither fcpt_exchange_unpack nor the boundary kernels
 * write (rows [8, nr-9)); the next fcpt_cfl / fcpt_cfl_device then only adds the rings next to the ghost zones
 * and reduces.  Same dt as the unsplit call.  A no-op whenever the interior is not yet final at that point
 * (damping outside the step kernels, fields uploaded since) -- the later call then does all rings. */
int fcpt_cfl_begin(fcpt_ctx *ctx);

/* sim::CalculateTimeStep's policy (src/simulation.cpp:100-118) applied to the
 * globally reduced CFL dt: returns min(CFLmaxVar*last_dt, cfl_dt) and stores it
 * as last_dt. */
int fcpt_calculate_timestep(fcpt_ctx *ctx, double cfl_dt_global, double *dt);

/* The monitor-time snapping of sim::run (src/simulation.cpp:528-540). */
int fcpt_snap_to_monitor(const fcpt_ctx *ctx, double cfl_dt, double *step_dt);

/* The gas part of one step.  Integrator: Euler -- step_Euler up to and including Transport (src/simulation.cpp:167-217):
 * potential, update_with_sourceterms, update_with_artificial_viscosity,
 * recalculate_viscosity, compute_viscous_stress_tensor,
 * update_velocities_with_viscosity, SubStep3, apply_boundary_condition(final=false),
 * Transport.  Integrator: Leapfrog -- step_LeapFrog (src/simulation.cpp:316-393): gas kick 1/2 with
 * dt/2, boundary (final=false), Transport with dt, potential at mid-step, compute_pressure,
 * gas kick 2/2 with dt/2.  Asynchronous on the context's stream.  Advances time by dt.
 *
 * The fused transport kernel handles |Nshift[i] - Nshift[i-1]| <= 1, which the FARGO shear term of the CFL
 * condition (src/cfl.cpp:207-220) makes the normal case; the two-kernel transport is queued behind it as a
 * device-side fallback and runs only when a ring pair exceeds that (a dt beyond the CFL step, or a source step
 * that changed v_phi violently), so every step is computed as the reference does.  FCPT_TRANSPORT_FALLBACK=0
 * (environment) drops the two idle launches for flows known to be benign; if the limit is then ever exceeded,
 * the next synchronising call returns FCPT_ESHEAR. */
int fcpt_step(fcpt_ctx *ctx, double dt);

/* CommunicateBoundaries, device side (src/commbound.cpp:108-125,163-180):
 * pack rows [7,14) -> send_inner and rows [nr-14,nr-7) -> send_outer of
 * Sigma, vrad, vazi(, energy); unpack recv_inner -> rows [0,7) and
 * recv_outer -> rows [nr-7,nr).  Buffers hold fcpt_exchange_count() doubles
 * each; device buffers take one copy kernel per call, host buffers one
 * hipMemcpyAsync per field and side; a NULL pointer skips that side.  The
 * transfer itself (RCCL send/recv between neighbouring slabs) is done by the
 * caller on the same stream. */
int fcpt_exchange_count(const fcpt_ctx *ctx, uint64_t *count);
int fcpt_exchange_pack(fcpt_ctx *ctx, double *send_inner, double *send_outer);
int fcpt_exchange_unpack(fcpt_ctx *ctx, const double *recv_inner, const double *recv_outer);

/* ---- radial slabs on several GPUs: RCCL inside the library ------------------------------------------
 * The reference's two communication points, on the context's stream (no host synchronisation, no stream hop):
 * CommunicateBoundaries' MPI_Isend/MPI_Irecv with CPU_Prev/CPU_Next (src/commbound.cpp:130-158) become one
 * group of ncclSend/ncclRecv with slab rank-1 / rank+1 over xGMI, condition_cfl's MPI_Allreduce(MPI_MIN)
 * (src/cfl.cpp:379) an ncclAllReduce(ncclMin) of one device double.  One process (or thread) per GPU, as one
 * MPI rank per slab in the reference (src/parallel.cpp:28-40).
 *
 * Bootstrap = ncclGetUniqueId on slab 0, the 128 bytes handed to every slab by the host's own means (the
 * reference's host would MPI_Bcast them; bench.py uses its torch.distributed store, the C++ driver a file),
 * then fcpt_comm_init on every slab (collective: ncclCommInitRank with rank = d->rank of d->nranks, on the
 * device the context was created on).  librccl is bound at run time; single-GPU users never load it. */
#define FCPT_COMM_ID_BYTES 128
int fcpt_comm_unique_id(void *id128);
int fcpt_comm_init(fcpt_ctx *ctx, const void *id128);
int fcpt_comm_destroy(fcpt_ctx *ctx);

/* The same communicator for ranks that cannot use RCCL among themselves -- several slabs on one GPU (RCCL refuses two
 * ranks on one device), i.e. rehearsals and tests of the N-rank path on a 1-GPU box, or more slabs than devices:
 * ghost rings and the CFL value are staged through pinned host memory and the shared-memory file `path` (collective
 * over the d->nranks slabs of ONE node; slab 0 creates the file, which must not belong to another run, and removes it
 * in fcpt_comm_destroy).  fcpt_exchange, fcpt_cfl_allreduce, fcpt_comm_barrier and fcpt_run_steps then work as with
 * fcpt_comm_init, but block the host in every transfer.  FCPT_HOSTLINK_TIMEOUT (seconds, default 120) bounds every
 * wait for another rank: FCPT_ECOMM afterwards. */
int fcpt_comm_init_host(fcpt_ctx *ctx, const char *path);

/* MPI_Barrier over the slabs of the communicator (src/main.cpp:141, the output routines): returns when every slab
 * has called it; the work queued on this context's stream before the call is complete then. */
int fcpt_comm_barrier(fcpt_ctx *ctx);

/* CommunicateBoundaries (src/commbound.cpp:98-182) of this slab, whole: pack rows [7,14) / [nr-14,nr-7),
 * grouped send/recv with the neighbours, unpack into rows [0,7) / [nr-7,nr).  Asynchronous.  With the option
 * comm_overlap the transfers run on the library's communication stream while the CFL terms of the interior
 * rings (fcpt_cfl_begin) are evaluated on the context's stream. */
int fcpt_exchange(fcpt_ctx *ctx);

/* condition_cfl's MPI_Allreduce (src/cfl.cpp:379), device-resident: queues the local reduction
 * (src/cfl.cpp:185-376) and the MIN over all slabs; the result stays in device memory, where
 * fcpt_calculate_timestep_device(ctx, NULL) picks it up.  With dt_global != NULL the call blocks and also
 * returns the value.  fcpt_run_steps uses both calls when the context has a communicator. */
int fcpt_cfl_allreduce(fcpt_ctx *ctx, double *dt_global);

/* ComputeDiskOnPlanetAccel's MPI_Allreduce(SUM) (src/Force.cpp:115): values[k] (host memory, in place, n <= 4 *
 * FCPT_MAX_BODIES) becomes the sum over the slabs of the communicator, the same bits on every slab -- each slab kicks
 * its own copy of the bodies with it.  Host-staged transport: every slab adds the slabs' values in rank order.  RCCL:
 * one ncclAllReduce(ncclSum), which hands every rank the one reduced value (this branch needs several GPUs and has not
 * been executed on the one-GPU machines the tests run on, like the rest of the RCCL path).  Blocks.  Without a
 * communicator: FCPT_OK, values untouched. */
int fcpt_allreduce_sum(fcpt_ctx *ctx, int32_t n, double *values);

/* The rest of step_Euler after CommunicateBoundaries (src/simulation.cpp:244-265):
 * apply_boundary_condition(final=true) (damping first) and
 * recalculate_derived_disk_quantities.  Asynchronous. */
int fcpt_post(fcpt_ctx *ctx, double dt);

/* boundary_conditions::apply_boundary_condition (src/boundary_conditions/boundary_conditions.cpp:65-114):
 * wave damping first when `final` is non-zero, then the eight per-variable ghost-ring
 * conditions.  Asynchronous.  (fcpt_step and fcpt_post call it internally; sim::init
 * calls it once more before the loop, src/simulation.cpp:463.) */
int fcpt_apply_boundary(fcpt_ctx *ctx, double dt, int32_t final);

/* K iterations of {cfl [+ MIN over the slabs], calculate_timestep, [snap], [particle step, [migration]], step,
 * [exchange], post} without returning to the caller, as sim::run does (src/simulation.cpp:515-553); the particle step
 * and, on several slabs, the migration with fcpt_particles_follow_run_steps.  A context with a communicator
 * (fcpt_comm_init) runs the multi-slab loop: every slab's host calls this with the same arguments.  If `snap` is non-zero the
 * step is snapped to monitor times and n_monitor advances.  nsteps_done may be
 * NULL.  Stops early when time reaches t_final = nsnapshots*nmonitor*monitor_timestep
 * unless t_final <= 0. */
int fcpt_run_steps(fcpt_ctx *ctx, int64_t nsteps, int32_t snap, int64_t *nsteps_done);

/* ---- measurement ----------------------------------------------------------- */

/* Per-kernel timing with HIP events recorded on the context's stream around each
 * launch of the kernels selected by `mask` (bit k = kernel id k, see
 * fcpt_kernel_name).  At most max_launches launches are recorded between start and
 * stop.  fcpt_profile_stop synchronises and fills ms_total[id] / launches[id]
 * (arrays of fcpt_kernel_count() entries).  Replaces nothing in the reference (its
 * only timer is the wall clock of hydro_dt_logger, src/hydro_dt_logger.h:13-34). */
int32_t fcpt_kernel_count(void);
const char *fcpt_kernel_name(int32_t id);
int fcpt_profile_start(fcpt_ctx *ctx, uint64_t mask, int32_t max_launches);
int fcpt_profile_stop(fcpt_ctx *ctx, double *ms_total, int64_t *launches);

/* Test hook, needs no GPU: the tables fcpt_transport_chunks / fcpt_source_chunks would report for a slab of nr x nphi
 * cells on a device of n_cu compute units (8 XCDs), isothermal or ideal EOS, with damping zones of damp_inner / damp_outer
 * rings folded into the transport.  n_transport / n_source = 0: equal chunks (small grids, rings of > 8192 cells ...). */
int fcpt_selftest_chunk_tables(int32_t nr, int32_t nphi, int32_t n_cu, int32_t adiabatic, int32_t damp_inner, int32_t damp_outer,
                               int32_t *transport_tile_first_last, int32_t transport_capacity, int32_t *n_transport,
                               int32_t *source_seg_first_last, int32_t source_capacity, int32_t *n_source);
/* Test hook, needs no GPU: one of the per-ring tables fcpt_create would upload for this descriptor and these global radii
 * (the slab of d->rank), as rows x cols doubles in row-major order.  Integer columns are converted; the columns of a
 * row table are the members of its row structure in declaration order (csrc/fcpt_internal.h).  `out` holds `capacity`
 * doubles (0 with out = NULL: only rows and cols are returned), nr = the slab's rings:
 *   FCPT_TABLE_SRC    nr + 8 rows, row m + 2 = iteration m of the marching source kernel (SrcRow, 40 columns)
 *   FCPT_TABLE_RAD    nr + 2 rows, row k + 1 = radial interface k (RadRow, 4 columns)
 *   FCPT_TABLE_THETA  nr rows (ThetaRow, 8 columns)
 *   FCPT_TABLE_DAMP   nr + 1 rows (DampRow, 10 columns: fs, ts, fv, tv, tvr, tva, tsg, ten, pad[0], pad[1])
 *   FCPT_TABLE_RING   nr + 2 rows, the plain per-ring arrays, each zero beyond its own length: cs_ring, nu_ring (nr);
 *                     g_dxtheta, g_inv_dxtheta, g_dr_invsurf, g_r_omega, g_inv_omk, g_omk (nr + 1, entry nr is 0);
 *                     g_ra3 (nr + 2); dfac_s, dtau_s, dfac_v, dtau_v, dtype_vr, dtype_va, dtype_sig, dtype_e (nr + 1);
 *                     ring_ref_damped (nr) -- 18 columns in this order
 *   FCPT_TABLE_DAMP_RANGES  9 rows of 6: row 2 q + o = (lo, hi, type, rlim, redge, tau) of field q (v_r, v_phi, Sigma, e)
 *                     at the inner (o = 0) or outer edge; row 8 = (damp_any, damp_foldable, 0, 0, 0, 0)
 *   FCPT_TABLE_AZIMUTH  nphi rows: cos(dphi j), sin(dphi j)
 *   FCPT_TABLE_TF     nr + 5 rows, row m + 3 = iteration m of the fused transport kernel (TfRow, 16 columns: dr_lo, dr_hi,
 *                     idr_up, invsurf, dxtheta, inv_dxtheta, invr, r_omega, r_next, romega_next, tvr, tva, tsg, ten, gphi,
 *                     dr_invsurf) */
enum { FCPT_TABLE_SRC = 0, FCPT_TABLE_RAD, FCPT_TABLE_THETA, FCPT_TABLE_DAMP, FCPT_TABLE_RING, FCPT_TABLE_DAMP_RANGES, FCPT_TABLE_AZIMUTH,
       FCPT_TABLE_TF };
int fcpt_selftest_ring_tables(const fcpt_desc *d, const double *radii, int32_t table, double *out, int64_t capacity,
                              int32_t *rows, int32_t *cols);
/* Test hook: out[k] = 0.5 * flux_limiter(a[k], b[k]) (src/TransportEuler.cpp:306-337; limiter = FCPT_LIMITER_*) exactly
 * as the transport kernels evaluate it on the device -- the van Leer form there is branch-free (max(ab, 0) times a
 * guarded reciprocal of a + b) and its edge cases (+-0, denormal and cancelling sums) are what this call lets a test
 * compare with `ab > 0 ? ab / (a + b) : 0`.  Host arrays of n doubles; blocks. */
int fcpt_selftest_half_limiter(int32_t limiter, int64_t n, const double *a, const double *b, double *out);

#ifdef __cplusplus
}
#endif
#endif /* FARGOCPT_HIP_H */
