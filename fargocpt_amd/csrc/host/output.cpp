// fargocpt_hip -- the output directory in the reference's format: the static files, the snapshots every slab writes
// its window of (write2D, src/polargrid.cpp:135-180) and the restart from one.
#include "driver.h"

#include <algorithm>
#include <cstring>
#include <fcntl.h>
#include <fstream>
#include <sys/stat.h>
#include <unistd.h>

void mkdirs(const std::string &p)
{
    std::string acc;
    for (size_t i = 0; i < p.size(); ++i) {
        acc += p[i];
        if (p[i] == '/' || i + 1 == p.size())
            mkdir(acc.c_str(), 0755);
    }
}

void die_cannot(const char *verb, const std::string &path)
{
    fprintf(stderr, "fargocpt_hip: cannot %s %s\n", verb, path.c_str());
    exit(1);
}
FILE *open_or_die(const std::string &path, const char *mode)
{
    FILE *f = fopen(path.c_str(), mode);
    if (!f)
        die_cannot(mode[0] == 'r' ? "read" : "write", path);
    return f;
}
// one slab's window of a file that exists (create_file + barrier): pwrite at the window's offset
static void write_window_or_die(const std::string &path, const void *data, size_t bytes, off_t offset)
{
    const int fd = open(path.c_str(), O_WRONLY);
    if (fd < 0 || pwrite(fd, data, bytes, offset) != (ssize_t)bytes)
        die_cannot("write", path);
    close(fd);
}

void barrier(const Driver &dr)
{
    if (dr.slab.multi())
        CHECK(fcpt_comm_barrier(dr.ctx));
}
void exchange(const Driver &dr)
{
    if (dr.slab.multi())
        CHECK(fcpt_exchange(dr.ctx));
}
// condition_cfl incl. its MPI_Allreduce(MIN) over the slabs (cfl.cpp:379) + CalculateTimeStep
double calc_dt(const Driver &dr)
{
    double cfl, dt;
    if (dr.slab.multi())
        CHECK(fcpt_cfl_allreduce(dr.ctx, &cfl));
    else
        CHECK(fcpt_cfl(dr.ctx, &cfl));
    CHECK(fcpt_calculate_timestep(dr.ctx, cfl, &dt));
    return dt;
}

static bool is_vector_field(int field) { return field == FCPT_F_VRAD || field == FCPT_F_VRAD0 || field == FCPT_F_MASSFLOW; }

// rank 0 creates / truncates the files of a collective write before the others open them
static void create_file(const std::string &path)
{
    FILE *f = fopen(path.c_str(), "wb");
    if (!f) {
        fprintf(stderr, "fargocpt_hip: cannot create %s\n", path.c_str());
        exit(1);
    }
    fclose(f);
}

// write2D (src/polargrid.cpp:135-180): raw FP64, global row-major; every slab writes its window at
// (IMIN + Zero_or_active) * Nsec.  Collective: the file exists (create_file + barrier) before this is called.
static void write_grid(const Driver &dr, int field, const std::string &path)
{
    const Slab &slab = dr.slab;
    const bool vec = is_vector_field(field);
    std::vector<double> buf(slab.local_count(vec));
    CHECK(fcpt_download(dr.ctx, field, buf.data()));
    int lo, hi;
    slab.window(vec, lo, hi);
    write_window_or_die(path, buf.data() + (size_t)lo * slab.nphi, (size_t)(hi - lo) * slab.nphi * sizeof(double),
                        (off_t)(slab.s.imin + lo) * slab.nphi * sizeof(double));
}

// t_polargrid::read2D (src/polargrid.cpp:301-353): raw doubles, ring-major; every slab takes its rows
// IMIN .. IMIN + NRadial (overlap rings included) out of the global file
static bool read_grid(const Driver &dr, int field, const std::string &path, bool required)
{
    const Slab &slab = dr.slab;
    const bool vec = is_vector_field(field);
    FILE *f = required ? open_or_die(path, "rb") : fopen(path.c_str(), "rb");
    if (!f)
        return false;
    const size_t n_global = (size_t)(slab.nr_global + (vec ? 1 : 0)) * slab.nphi, n = slab.local_count(vec);
    fseek(f, 0, SEEK_END);
    const size_t have = (size_t)ftell(f) / sizeof(double);
    if (have != n_global) {
        fprintf(stderr, "fargocpt_hip: %s holds %zu values, expected %zu (Nrad / Naz changed?)\n", path.c_str(), have, n_global);
        exit(1);
    }
    std::vector<double> buf(n);
    fseek(f, (long)((size_t)slab.s.imin * slab.nphi * sizeof(double)), SEEK_SET);
    const size_t got = fread(buf.data(), sizeof(double), n, f);
    fclose(f);
    if (got != n) {
        fprintf(stderr, "fargocpt_hip: short read of %s\n", path.c_str());
        exit(1);
    }
    CHECK(fcpt_upload(dr.ctx, field, buf.data()));
    return true;
}

// boundary_conditions::initial_values_needed(): the t = 0 grids are part of the state (damping towards them,
// reference boundary conditions)
bool needs_reference(const fcpt_desc &d)
{
    bool needs = d.damping != 0;
    for (int sd = 0; sd < 2; ++sd)
        needs = needs || d.bc_sigma[sd] == FCPT_BC_REFERENCE || d.bc_energy[sd] == FCPT_BC_REFERENCE ||
                d.bc_vrad[sd] == FCPT_BC_REFERENCE || d.bc_vaz[sd] == FCPT_BC_REFERENCE;
    return needs;
}

// used_rad.dat, dimensions.dat, units.yml and info2D.yml of a fresh run; the snapshot list starts empty
void write_static_files(const Driver &dr)
{
    const fcpt_desc &d = dr.desc;
    FILE *f = open_or_die(dr.outdir + "used_rad.dat", "w"); // src/init.cpp:228-246
    for (int n = 0; n <= d.nr_global; ++n)
        fprintf(f, "%.18g\n", dr.radii[n]);
    fclose(f);
    f = open_or_die(dr.outdir + "dimensions.dat", "w"); // src/parameters.cpp:1127-1176
    const char *sp[] = {"Arithmetic", "Logarithmic", "Exponential"};
    fprintf(f, "#RMIN\tRMAX\tPHIMIN\tPHIMAX          \tNRAD\tNAZ\tNGHRAD\tNGHAZ\tRadial_spacing\n");
    fprintf(f, "%.16g\t%.16g\t%.16g\t%.16g\t%d\t%d\t%d\t%d\t%s\n", d.rmin, d.rmax, 0.0, 2 * M_PI, d.nr_global, d.nphi, 1,
            1, sp[d.radial_spacing]);
    fclose(f);
    remove((dr.outdir + "snapshots/list.txt").c_str());
    // units.yml (write_code_units_file, src/units.cpp:449-497) and info2D.yml (src/output.cpp:786-846):
    // what the reference's Python loader (python_module/fargocpt/data.py) needs beside the grids
    const double len = dr.units.L0, mass = dr.units.M0, tim = dr.units.TIME0, temp = dr.units.TEMP0;
    const double energy = len * len * mass / (tim * tim), vel = len / tim;
    struct U {
        const char *name, *sym;
        double v;
    };
    const U units[] = {
        {"length", "cm", len},
        {"mass", "g", mass},
        {"time", "s", tim},
        {"temperature", "K", temp},
        {"energy", "erg", energy},
        {"energy surface density", "erg cm^-2", mass / (tim * tim)},
        {"density", "g cm^-3", mass / (len * len * len)},
        {"mass surface density", "g cm^-2", mass / (len * len)},
        {"opacity", "g^-1 cm^2", len * len / mass},
        {"energy flux", "erg cm^-2 s^-1", energy / (len * len * tim)},
        {"velocity", "cm s^-1", vel},
        {"angular momentum", "cm^2 g s^-1", len * mass * vel},
        {"kinematic viscosity", "cm^2 s^-1", len * len / tim},
        {"dynamic viscosity", "P", mass / (len * tim)},
        {"acceleration", "cm s^-2", len / (tim * tim)},
        {"stress", "g s^-2", mass / (tim * tim)},
        {"pressure", "dyn cm^-1", mass / (tim * tim)},
        {"power", "erg/s", mass * len * len / (tim * tim * tim)},
        {"potential", "erg/g", len * len / (tim * tim)},
        {"torque", "erg", len * len * mass / (tim * tim)},
        {"force", "dyn", mass * len / (tim * tim)},
        {"mass accretion rate", "g s^-1", mass / tim},
    };
    f = open_or_die(dr.outdir + "units.yml", "w");
    fprintf(f, "# code units file\n# version 0.2\n\n");
    for (const U &u : units)
        fprintf(f, "%s:\n  cgs symbol: %s\n  cgs value: %.17g\n  unit: %.17g %s\n\n", u.name, u.sym, u.v, u.v, u.sym);
    fclose(f);
    struct G {
        const char *name, *sym;
        double v;
        bool vec;
    };
    const G grids[] = {{"Sigma", "g cm^-2", mass / (len * len), false},
                       {"vrad", "cm s^-1", vel, true},
                       {"vazi", "cm s^-1", vel, false},
                       {"energy", "erg cm^-2", mass / (tim * tim), false},
                       {"Temperature", "K", temp, false},
                       {"a_sg_rad", "cm s^-2", len / (tim * tim), false},
                       {"a_sg_azi", "cm s^-2", len / (tim * tim), false}};
    f = open_or_die(dr.outdir + "info2D.yml", "w");
    fprintf(f, "# 2D output variable descriptions\n# version 0.1\n\n");
    for (const G &g : grids) {
        if ((!strcmp(g.name, "energy") || !strcmp(g.name, "Temperature")) && d.eos != FCPT_EOS_IDEAL)
            continue;
        if ((!strcmp(g.name, "a_sg_rad") && !(dr.sg.on && dr.sg.write_rad)) || (!strcmp(g.name, "a_sg_azi") && !(dr.sg.on && dr.sg.write_azi)))
            continue;
        fprintf(f, "%s:\n  cgs symbols: %s\n  code_to_cgs_factor: %.17g\n  unit: %.17g %s\n  Nrad: %d\n  Nazi: %d\n",
                g.name, g.sym, g.v, g.v, g.sym, g.vec ? d.nr_global + 1 : d.nr_global, d.nphi);
        fprintf(f, "  bigendian: 0\n  on_radial_interface: %s\n  on_azimuthal_interface: %s\n  filename: %s.dat\n\n",
                g.vec ? "true" : "false", !strcmp(g.name, "vazi") ? "true" : "false", g.name);
    }
    fclose(f);
}

// The grids of a snapshot, for its writer and for restart_load.  field0: the t = 0 copy that the "reference" snapshot
// restores, or -1.  A restart needs the grid (2), takes it if it is there (1) or recomputes it (0).
struct SnapshotGrid {
    int field, field0;
    const char *file;
    int restart;
};
static std::vector<SnapshotGrid> snapshot_grids(const Driver &dr)
{
    const fcpt_desc &d = dr.desc;
    std::vector<SnapshotGrid> grids = {{FCPT_F_SIGMA, FCPT_F_SIGMA0, "Sigma.dat", 2},
                                       {FCPT_F_VRAD, FCPT_F_VRAD0, "vrad.dat", 2},
                                       {FCPT_F_VAZI, FCPT_F_VAZI0, "vazi.dat", 2}};
    if (d.eos == FCPT_EOS_IDEAL) {
        grids.push_back({FCPT_F_ENERGY, FCPT_F_ENERGY0, "energy.dat", 2});
        grids.push_back({FCPT_F_TEMPERATURE, -1, "Temperature.dat", 0});
        // the CFL condition of the next step reads Q+ and Q- of the last one (cfl.cpp:303-316): restart.cpp:78-95
        grids.push_back({FCPT_F_QPLUS, -1, "Qplus.dat", 1});
        grids.push_back({FCPT_F_QMINUS, -1, "Qminus.dat", 1});
    }
    // WriteSGAccelRad / WriteSGAccelAzi (data.cpp:61-68): what the last kick's compute left; a restart recomputes them
    if (dr.sg.on && dr.sg.write_rad)
        grids.push_back({FCPT_F_SG_ACCEL_RAD, -1, "a_sg_rad.dat", 0});
    if (dr.sg.on && dr.sg.write_azi)
        grids.push_back({FCPT_F_SG_ACCEL_AZI, -1, "a_sg_azi.dat", 0});
    return grids;
}

// MassFlow1D.dat (t_polargrid::write1D, polargrid.cpp:187-278, of a vector grid that is integrated over
// azimuth): pairs (Rinf[n], sum_j MASSFLOW(n, j) / (Nmonitor MonitorTimestep)) -- calculate_massflow,
// quantities.cpp:770-781 -- every slab its window of interfaces at (IMIN + Zero_or_active) * 2, then the
// grid is cleared (data.cpp:277)
static void write_massflow(const Driver &dr, const std::string &path)
{
    const fcpt_desc &d = dr.desc;
    const Slab &slab = dr.slab;
    std::vector<double> mf(slab.local_count(true));
    CHECK(fcpt_download(dr.ctx, FCPT_F_MASSFLOW, mf.data()));
    int lo, hi;
    slab.window(true, lo, hi);
    std::vector<double> out(2 * (size_t)(hi - lo));
    const double denom = (double)d.nmonitor * d.monitor_timestep;
    for (int n = lo; n < hi; ++n) {
        double sum = 0.0;
        for (int j = 0; j < d.nphi; ++j)
            sum += mf[(size_t)n * d.nphi + j] / denom;
        out[2 * (size_t)(n - lo)] = dr.radii[slab.s.imin + n];
        out[2 * (size_t)(n - lo) + 1] = sum;
    }
    write_window_or_die(path, out.data(), out.size() * sizeof(double), (off_t)(slab.s.imin + lo) * 2 * sizeof(double));
    std::fill(mf.begin(), mf.end(), 0.0);
    CHECK(fcpt_upload(dr.ctx, FCPT_F_MASSFLOW, mf.data()));
}

void write_snapshot(const Driver &dr, const BodySystem &bs, Particles &pt, unsigned nsnap, unsigned nmon, const char *name)
{
    const fcpt_desc &d = dr.desc;
    fcpt_clock clk;
    CHECK(fcpt_get_clock(dr.ctx, &clk));
    const std::string dir = dr.outdir + "snapshots/" + (name ? std::string(name) : std::to_string(nsnap)) + "/";
    const std::vector<SnapshotGrid> grids = snapshot_grids(dr);
    const bool massflow = d.write_massflow && !name;
    // MPI_File_open(MPI_MODE_CREATE) is collective in the reference; here rank 0 creates the directory and the
    // empty files, then every slab writes its window into them
    if (dr.slab.master()) {
        mkdirs(dir);
        for (const SnapshotGrid &g : grids)
            create_file(dir + g.file);
        if (massflow)
            create_file(dir + "MassFlow1D.dat");
    }
    barrier(dr);
    for (const SnapshotGrid &g : grids)
        write_grid(dr, g.field, dir + g.file);
    if (massflow)
        write_massflow(dr, dir + "MassFlow1D.dat");
    barrier(dr); // the grids are complete before misc.bin and list.txt announce the snapshot
    if (!dr.slab.master())
        return;
    if (bs.free)
        bs.save(dir);
    if (pt.ps.on && !name)
        pt.write(dir);
    misc_entry misc;
    memset(&misc, 0, sizeof(misc));
    misc.timestep = nsnap;
    misc.nTimeStep = nmon;
    misc.time = clk.time;
    misc.OmegaFrame = d.omega_frame;
    misc.last_dt = clk.last_dt;
    misc.N_iter = clk.n_hydro_iter;
    FILE *f = open_or_die(dir + "misc.bin", "wb"); // src/output.cpp:494-527
    fwrite(&misc, sizeof(misc), 1, f);
    fclose(f);
    std::ifstream src(dr.cfgpath, std::ios::binary);
    std::ofstream dst(dir + "config.yml", std::ios::binary);
    dst << src.rdbuf();
    if (name)
        return; // write_full_output(data, "reference", false): not registered
    f = open_or_die(dr.outdir + "snapshots/list.txt", "a");
    fprintf(f, "%u\n", nsnap);
    fclose(f);
    f = open_or_die(dr.outdir + "snapshots/timeSnapshot.dat", nsnap == 0 ? "w" : "a");
    if (nsnap == 0)
        fprintf(f, "# Time log for course output.\n#version: 0.1\n#variable: 0 | snapshot number | 1\n"
                   "#variable: 1 | monitor number | 1\n#variable: 2 | time | code\n");
    fprintf(f, "%u\t%u\t%#.16e\n", nsnap, nmon, clk.time);
    fclose(f);
    if (!dr.quiet)
        printf("Writing output %s, Snapshot Number %u, Time %f.\n", dir.c_str(), nsnap, clk.time);
}

// restart_load, src/restart.cpp:18-139: the state of the snapshot in restart_dir into the context, the bodies and the
// particles; returns the snapshot's misc.bin
misc_entry restart_load(const Driver &dr, BodySystem &bs, Particles &pt, const std::string &restart_dir)
{
    misc_entry misc;
    FILE *mf = open_or_die(restart_dir + "misc.bin", "rb");
    if (fread(&misc, sizeof(misc), 1, mf) != 1)
        die_cannot("read", restart_dir + "misc.bin");
    fclose(mf);
    const std::vector<SnapshotGrid> grids = snapshot_grids(dr);
    if (needs_reference(dr.desc))
        for (const SnapshotGrid &g : grids)
            if (g.field0 >= 0)
                read_grid(dr, g.field0, dr.outdir + "snapshots/reference/" + g.file, true);
    bool bitwise = true;
    for (const SnapshotGrid &g : grids)
        if (g.restart)
            bitwise = read_grid(dr, g.field, restart_dir + g.file, g.restart == 2) && bitwise;
    if (!bitwise && !dr.quiet)
        printf("Cannot read Qplus / Qminus, no bitwise identical restarting possible!\n");
    fcpt_clock clk;
    CHECK(fcpt_get_clock(dr.ctx, &clk));
    clk.time = misc.time;
    clk.last_dt = misc.last_dt;
    clk.n_hydro_iter = misc.N_iter;
    clk.n_monitor = misc.nTimeStep;
    clk.n_snapshot = misc.timestep;
    CHECK(fcpt_set_clock(dr.ctx, &clk));
    if (bs.free)
        bs.load(restart_dir);
    bs.set(misc.time);
    CHECK(fcpt_recalculate_derived(dr.ctx));
    if (pt.ps.on)
        pt.read(restart_dir);
    if (!dr.quiet)
        printf("Restarting from %s at time %f (snapshot %u, monitor step %u).\n", restart_dir.c_str(), misc.time,
               misc.timestep, misc.nTimeStep);
    return misc;
}
