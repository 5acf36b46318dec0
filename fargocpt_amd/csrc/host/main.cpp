// fargocpt_hip -- host driver over the C ABI: reads a FargoCPT YAML setup, runs the gas update
// on the GPU with the reference's main loop and writes snapshots in the reference's format.
//
//   fargocpt_hip [-q] [--lenient] [-N <steps>] [--ranks <n>] [--transport auto|rccl|host] start|auto|restart [N] <config.yml>
//
// --ranks n: the reference's `mpirun -np n fargocpt_exe ...` (src/parallel.cpp:28-40, one MPI rank per radial slab):
// this process starts n copies of itself -- before anything touches a GPU -- one per slab and GPU, and waits for
// them; the slabs exchange their ghost rings and the CFL minimum through the library (RCCL when every rank has a GPU
// of its own, the host-staged transport otherwise, e.g. 2 or 3 ranks on a 1-GPU box) and write their windows of the
// snapshot files as write2D does (src/polargrid.cpp:135-180).  A launcher of one's own sets FCPT_RANK, FCPT_NRANKS
// and FCPT_RDV (a directory all ranks see) instead.
//
// Counterpart of src/main.cpp:47-164 + sim::run (src/simulation.cpp:505-558) +
// handle_outputs (:50-98) for the gas path only.  Without --bodies free N-body objects do not feel anything here
// (no REBOUND, no disk feedback): the star sits at the origin and every planet moves on its
// initial circular orbit, seen in the frame rotating with OmegaFrame.
//
// main() is the list of the stages, in the order that is the behaviour: which refusal a setup meets first, and that
// none of them needs a GPU, follows from where each stage stands.  The setup and its units are in config.cpp, the
// bodies in bodies.cpp, the dust particles in particles.cpp, the files in output.cpp and the loop in run.cpp.
#include "driver.h"

#include <algorithm>
#include <cerrno>
#include <fstream>
#include <signal.h>
#include <sys/stat.h>
#include <sys/wait.h>
#include <unistd.h>

namespace {

struct Options {
    bool quiet = false, lenient = false;
    long max_steps = -1, restart_from = -1;
    int want_ranks = 1;
    bool have_dust_seed = false;
    unsigned long long dust_seed = 0;
    std::string mode, cfgpath, transport = "auto", bodies_mode = "circular";
};

Options parse_command_line(int argc, char **argv)
{
    Options o;
    bool bad_dust_seed = false;
    for (int i = 1; i < argc; ++i) {
        const std::string a = argv[i];
        if (a == "--dust-seed") { // unsigned 64-bit, decimal: the key of the diffusion kicks' generator
            const std::string v = i + 1 < argc ? argv[++i] : "";
            char *end = nullptr;
            errno = 0;
            o.dust_seed = strtoull(v.c_str(), &end, 10);
            bad_dust_seed = v.empty() || v.find_first_not_of("0123456789") != std::string::npos || errno == ERANGE || *end;
            o.have_dust_seed = true;
        } else if (a == "-q")
            o.quiet = true;
        else if (a == "--lenient")
            o.lenient = true;
        else if ((a == "--ranks" || a == "-np") && i + 1 < argc)
            o.want_ranks = atoi(argv[++i]);
        else if (a == "--transport" && i + 1 < argc)
            o.transport = lower(argv[++i]);
        else if (a == "--bodies" && i + 1 < argc)
            o.bodies_mode = lower(argv[++i]);
        else if (a == "-N" && i + 1 < argc)
            o.max_steps = atol(argv[++i]);
        else if (o.mode.empty())
            o.mode = a;
        else if (o.mode == "restart" && o.restart_from < 0 && !a.empty() && a.find_first_not_of("0123456789") == std::string::npos)
            o.restart_from = atol(a.c_str());
        else
            o.cfgpath = a;
    }
    // start_mode.cpp:29-113: start | restart [N] | auto
    if ((o.mode != "start" && o.mode != "restart" && o.mode != "auto") || o.cfgpath.empty() || o.want_ranks < 1 ||
        (o.transport != "auto" && o.transport != "rccl" && o.transport != "host") ||
        (o.bodies_mode != "circular" && o.bodies_mode != "free") || bad_dust_seed) {
        if (bad_dust_seed)
            fprintf(stderr, "fargocpt_hip: --dust-seed needs an unsigned 64-bit integer\n");
        fprintf(stderr, "usage: fargocpt_hip [-q] [--lenient] [-N steps] [--ranks n] [--transport auto|rccl|host] "
                        "[--bodies circular|free] [--dust-seed N] start|auto|restart [N] <config.yml>\n");
        exit(2);
    }
    return o;
}

// this process's rank: FCPT_RANK / FCPT_NRANKS from the --ranks parent or from a launcher of the caller's; false if
// the environment names none
bool rank_from_environment(int want_ranks, Slab &slab)
{
    const char *env_rank = getenv("FCPT_RANK"), *env_nranks = getenv("FCPT_NRANKS");
    if (!(env_rank && env_nranks))
        return false;
    slab.rank = atoi(env_rank);
    slab.nranks = atoi(env_nranks);
    if (slab.nranks < 1 || slab.rank < 0 || slab.rank >= slab.nranks) {
        fprintf(stderr, "fargocpt_hip: FCPT_RANK=%s FCPT_NRANKS=%s\n", env_rank, env_nranks);
        exit(2);
    }
    if (want_ranks > 1 && want_ranks != slab.nranks) {
        fprintf(stderr, "fargocpt_hip: --ranks %d but FCPT_NRANKS=%d\n", want_ranks, slab.nranks);
        exit(2);
    }
    return true;
}

// --bodies free: the bodies move under their own gravity (fcpt_nbody_*) and, with DiskFeedback, under the disk's;
// what that mode does not cover is refused here, before any device is asked for
void check_bodies_mode(const Config &cfg, const Driver &dr, BodySystem &bs)
{
    bs.disk_feedback = cfg.flag("DiskFeedback", true); // parameters.cpp:788
    if (bs.free && dr.desc.integrator != FCPT_INTEGRATOR_EULER) {
        fprintf(stderr, "fargocpt_hip: --bodies free needs Integrator: Euler (the drift-kick-drift of the bodies in "
                        "step_LeapFrog is not implemented)\n");
        exit(2);
    }
    if (bs.free && lower(cfg.str("HydroFrameCenter", "primary")) != "primary") {
        fprintf(stderr, "fargocpt_hip: --bodies free needs HydroFrameCenter: primary\n");
        exit(2);
    }
    if (bs.free && cfg.nbody.size() > FCPT_MAX_BODIES) {
        fprintf(stderr, "fargocpt_hip: --bodies free: more than %d bodies\n", FCPT_MAX_BODIES);
        exit(2);
    }
    if (!bs.free && cfg.has("DiskFeedback") && bs.disk_feedback && !dr.quiet)
        fprintf(stderr, "fargocpt_hip: note: DiskFeedback: yes is not applied with --bodies circular (the bodies keep "
                        "their circular orbits); --bodies free applies it\n");
}

// The parent of `--ranks n`: starts n copies of this program, one per slab, before anything here has touched a GPU
// (fork + exec at once), hands them FCPT_RANK / FCPT_NRANKS / FCPT_RDV (a fresh rendezvous directory under the output
// directory: the RCCL id or the shared-memory file of the host-staged transport), and waits for all of them.  The
// first rank that fails ends the others -- they would wait for it in a collective -- with SIGTERM to exactly the
// children started here.
int launch_ranks(int n, const std::string &outdir, bool quiet, char **argv)
{
    mkdirs(outdir);
    const std::string rdv = outdir + ".fcpt_rdv_" + std::to_string((long)getpid());
    mkdir(rdv.c_str(), 0700);
    std::vector<pid_t> pids((size_t)n, (pid_t)-1);
    for (int r = 0; r < n; ++r) {
        const pid_t pid = fork();
        if (pid < 0) {
            perror("fargocpt_hip: fork");
            for (int k = 0; k < r; ++k)
                kill(pids[k], SIGTERM);
            return 1;
        }
        if (pid == 0) {
            setenv("FCPT_RANK", std::to_string(r).c_str(), 1);
            setenv("FCPT_NRANKS", std::to_string(n).c_str(), 1);
            setenv("FCPT_RDV", rdv.c_str(), 1);
            setenv("HSA_ENABLE_IPC_MODE_LEGACY", "0", 0); // dmabuf IPC: what RCCL needs between processes on this driver
            execv("/proc/self/exe", argv);
            perror("fargocpt_hip: execv");
            _exit(127);
        }
        pids[r] = pid;
    }
    int failed = 0, alive = n;
    double t_term = 0.0;
    auto now = [] { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); };
    while (alive > 0) {
        bool progress = false;
        for (int r = 0; r < n; ++r) {
            if (pids[r] < 0)
                continue;
            int st = 0;
            const pid_t w = waitpid(pids[r], &st, WNOHANG);
            if (w != pids[r])
                continue;
            progress = true;
            pids[r] = -1;
            --alive;
            const int rc = WIFEXITED(st) ? WEXITSTATUS(st) : 128 + (WIFSIGNALED(st) ? WTERMSIG(st) : 0);
            if (rc != 0 && !failed) {
                failed = rc;
                fprintf(stderr, "fargocpt_hip: rank %d ended with code %d: ending the other ranks\n", r, rc);
                for (int k = 0; k < n; ++k)
                    if (pids[k] > 0)
                        kill(pids[k], SIGTERM);
                t_term = now();
            }
        }
        if (failed && alive > 0 && now() - t_term > 10.0) {
            for (int k = 0; k < n; ++k)
                if (pids[k] > 0)
                    kill(pids[k], SIGKILL);
            t_term = now() + 1e9;
        }
        if (!progress)
            usleep(2000);
    }
    for (const char *f : {"/rccl_id", "/rccl_id.tmp", "/hostlink"})
        unlink((rdv + f).c_str());
    rmdir(rdv.c_str());
    if (!quiet && !failed)
        printf("fargocpt_hip: %d ranks finished\n", n);
    return failed ? 1 : 0;
}

// start_mode::configure_start_mode (src/start_mode.cpp:29-113): auto = restart from the last snapshot of
// snapshots/list.txt if there is one; restart without a number likewise.  The directory to restart from, or "".
std::string start_mode(const Options &opt, const Driver &dr)
{
    if (opt.mode == "start")
        return "";
    std::string id = opt.restart_from >= 0 ? std::to_string(opt.restart_from) : "";
    if (id.empty()) {
        std::ifstream list(dr.outdir + "snapshots/list.txt");
        std::string line;
        while (std::getline(list, line))
            if (!line.empty())
                id = line; // output::get_last_snapshot_id
    }
    FILE *mf = id.empty() ? nullptr : fopen((dr.outdir + "snapshots/" + id + "/misc.bin").c_str(), "rb");
    if (mf) {
        fclose(mf);
        return dr.outdir + "snapshots/" + id + "/";
    }
    if (opt.mode == "restart" && opt.restart_from >= 0)
        die_cannot("read", dr.outdir + "snapshots/" + id + "/misc.bin");
    if (!dr.quiet)
        printf("No output found, starting fresh simulation\n");
    return "";
}

struct GlobalFields {
    std::vector<double> sigma, vrad, vazi, energy;
};

// The initial fields of the GLOBAL grid (rank 0 of 1), of which every slab then takes its rows IMIN .. IMIN + NRadial:
// the reference fills each rank's rows from the same formulas of the global ring index, and the one global quantity
// of init_physics -- SetSigma0's disk mass, an MPI sum there -- is then the same number on every rank by construction
GlobalFields initial_fields(const Config &cfg, Driver &dr)
{
    fcpt_desc &d = dr.desc;
    dr.radii.resize(d.nr_global + FCPT_GEOM_PAD + 1);
    CHECK(fcpt_radii(&d, dr.radii.data()));
    const size_t ns = (size_t)d.nr_global * d.nphi, nv = (size_t)(d.nr_global + 1) * d.nphi;
    GlobalFields g{std::vector<double>(ns), std::vector<double>(nv), std::vector<double>(ns), std::vector<double>(ns)};
    d.rank = 0;
    d.nranks = 1;
    CHECK(fcpt_initial_fields(&d, dr.radii.data(), g.sigma.data(), g.vrad.data(), g.vazi.data(), g.energy.data()));
    // SigmaCondition / EnergyCondition: 2D (init.cpp:1002-1007,1307-1312: read2D of the named file); 1D needs the
    // reference's GSL spline and is not offered
    for (int q = 0; q < 2; ++q) {
        const std::string cond = lower(cfg.str(q == 0 ? "SigmaCondition" : "EnergyCondition", "profile"));
        const std::string fn = cfg.str(q == 0 ? "SigmaFilename" : "EnergyFilename", "");
        if (cond == "profile" || cond.empty())
            continue;
        if (cond != "2d" || (q == 1 && d.eos != FCPT_EOS_IDEAL)) {
            if (q == 1 && cond == "2d")
                continue; // no energy equation
            fprintf(stderr, "fargocpt_hip: %sCondition: %s is not supported (Profile, 2D)\n", q == 0 ? "Sigma" : "Energy", cond.c_str());
            exit(2);
        }
        if (d.set_sigma0 || d.profile_cutoff_inner || d.profile_cutoff_outer) {
            fprintf(stderr, "fargocpt_hip: %sCondition: 2D together with SetSigma0 or ProfileCutoff* is not supported\n", q == 0 ? "Sigma" : "Energy");
            exit(2);
        }
        std::vector<double> &dst = q == 0 ? g.sigma : g.energy;
        FILE *f = fopen(fn.c_str(), "rb");
        if (!f || fread(dst.data(), sizeof(double), ns, f) != ns) {
            fprintf(stderr, "fargocpt_hip: cannot read %zu values from '%s'\n", ns, fn.c_str());
            exit(1);
        }
        fclose(f);
    }
    return g;
}

// This rank's slab, its GPU and its context (SplitDomain, src/split.cpp:34-88; src/parallel.cpp:28-40), with its rows of
// the global fields.  Settles --transport auto; returns the number of devices.
// fcpt_device_count is the first call of the driver that can open a device: the --ranks parent has returned before
// it, and so has every exit of the stages above, which is how they run on a machine without a GPU.
int create_on_device(Driver &dr, GlobalFields &g, std::string &transport)
{
    fcpt_desc &d = dr.desc;
    Slab &slab = dr.slab;
    d.rank = slab.rank;
    d.nranks = slab.nranks;
    CHECK(fcpt_split_domain(&d, &slab.s));
    slab.nphi = d.nphi;
    slab.nr_global = d.nr_global;
    int32_t ndev = 0;
    CHECK(fcpt_device_count(&ndev));
    if (ndev <= 0) {
        fprintf(stderr, "fargocpt_hip: no HIP device: the gas update has no CPU path\n");
        exit(1);
    }
    if (transport == "auto")
        transport = slab.nranks <= ndev ? "rccl" : "host";
    if (slab.multi() && transport == "rccl" && slab.nranks > ndev) {
        fprintf(stderr, "fargocpt_hip: --transport rccl needs one GPU per rank (%d ranks, %d GPU(s)): RCCL refuses two "
                        "ranks on one device\n", slab.nranks, (int)ndev);
        exit(2);
    }
    CHECK(fcpt_set_device(slab.rank % ndev));
    CHECK(fcpt_create(&d, dr.radii.data(), &dr.ctx));
    const size_t row0 = (size_t)slab.s.imin * d.nphi; // local row 0 = global row IMIN
    CHECK(fcpt_upload(dr.ctx, FCPT_F_SIGMA, g.sigma.data() + row0));
    CHECK(fcpt_upload(dr.ctx, FCPT_F_VRAD, g.vrad.data() + row0));
    CHECK(fcpt_upload(dr.ctx, FCPT_F_VAZI, g.vazi.data() + row0));
    CHECK(fcpt_upload(dr.ctx, FCPT_F_ENERGY, g.energy.data() + row0));
    g = GlobalFields(); // the global copies are not needed any more
    return ndev;
}

// The communicator of the slabs, over the rendezvous directory FCPT_RDV
void connect_ranks(const Driver &dr, const std::string &transport, int ndev)
{
    const Slab &slab = dr.slab;
    const char *e = getenv("FCPT_RDV");
    const std::string rdv = e && e[0] ? std::string(e) : dr.outdir + ".fcpt_rdv";
    if (slab.master())
        mkdirs(rdv + "/");
    if (transport == "host") {
        CHECK(fcpt_comm_init_host(dr.ctx, (rdv + "/hostlink").c_str()));
    } else {
        // ncclGetUniqueId on slab 0; the 128 bytes travel by file (the reference's host would MPI_Bcast them)
        unsigned char id[FCPT_COMM_ID_BYTES];
        const std::string idf = rdv + "/rccl_id";
        if (slab.master()) {
            CHECK(fcpt_comm_unique_id(id));
            FILE *f = fopen((idf + ".tmp").c_str(), "wb");
            if (!f || fwrite(id, 1, sizeof(id), f) != sizeof(id) || fclose(f) != 0 || rename((idf + ".tmp").c_str(), idf.c_str()) != 0)
                die_cannot("write", idf);
        } else {
            const auto t0 = std::chrono::steady_clock::now();
            for (;;) {
                FILE *f = fopen(idf.c_str(), "rb");
                const bool ok = f && fread(id, 1, sizeof(id), f) == sizeof(id);
                if (f)
                    fclose(f);
                if (ok)
                    break;
                if (std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count() > 120.0) {
                    fprintf(stderr, "fargocpt_hip: rank %d: no RCCL id in %s after 120 s\n", slab.rank, idf.c_str());
                    exit(1);
                }
                usleep(2000);
            }
        }
        CHECK(fcpt_comm_init(dr.ctx, id));
    }
    if (!dr.quiet)
        printf("fargocpt_hip: %d radial slabs, %s transport, %d GPU(s) visible\n", slab.nranks,
               transport == "host" ? "host-staged" : "RCCL", ndev);
}

// selfgravity::init (selfgravity.cpp:219-301): the kernel spectra and one compute(data, 0, false); every kick of the
// library's step then begins with the self-gravity kick.  A fresh run also takes the initial v_phi of a self-gravitating
// disk (init.cpp:1720-1746 with selfgravity::init_azimuthal_velocity, selfgravity.cpp:749-781): in rows 0 .. Nr-2
//   v_phi = Rmed sqrt(omega_cell^2 - <g_r> / Rmed) - OmegaFrame Rmed,   omega_cell = v_phi0 / Rmed,
// with <g_r> the ring mean and v_phi0 the speed without self-gravity, which fcpt_initial_fields has left (minus the
// frame's) in the grid; the last row stays at the frame's speed alone until the boundary call.  A restart stores nothing
// extra: the velocities come from the snapshot, the accelerations are recomputed by the first kick.
void init_selfgravity(Driver &dr, bool restarting)
{
    const fcpt_desc &d = dr.desc;
    const fcpt_selfgravity_params p = {dr.sg.mode, 1, dr.sg.aspect_ratio, dr.sg.thickness_smoothing_sg};
    CHECK(fcpt_selfgravity(dr.ctx, &p));
    CHECK(fcpt_selfgravity_compute(dr.ctx));
    if (restarting)
        return;
    const int nr = d.nr_global, nphi = d.nphi;
    std::vector<double> g_r((size_t)nr * nphi), vazi((size_t)nr * nphi);
    CHECK(fcpt_download(dr.ctx, FCPT_F_SG_ACCEL_RAD, g_r.data()));
    CHECK(fcpt_download(dr.ctx, FCPT_F_VAZI, vazi.data()));
    for (int i = 0; i < nr; ++i) {
        const double ri = dr.radii[i], rs = dr.radii[i + 1];
        double rmed = 2.0 / 3.0 * (rs * rs * rs - ri * ri * ri);
        rmed = rmed / (rs * rs - ri * ri);
        double mean = 0.0; // mpi_make1Dprofile: the plain sum over the ring, divided by Nphi
        for (int j = 0; j < nphi; ++j)
            mean += g_r[(size_t)i * nphi + j];
        mean /= (double)nphi;
        for (int j = 0; j < nphi; ++j) {
            double &v = vazi[(size_t)i * nphi + j];
            if (i == nr - 1) {
                v = -d.omega_frame * rmed;
                continue;
            }
            const double omega_cell = (v + d.omega_frame * rmed) / rmed;
            const double temp = omega_cell * omega_cell - mean / rmed;
            if (temp < 0 && j == 0)
                fprintf(stderr, "fargocpt_hip: Radicand %g < 0 in init_azimuthal_velocity! Maybe ThicknessSmoothingSG (%g) is too small!\n",
                        temp, dr.sg.thickness_smoothing_sg);
            v = rmed * std::sqrt(temp) - d.omega_frame * rmed;
        }
    }
    CHECK(fcpt_upload(dr.ctx, FCPT_F_VAZI, vazi.data()));
}

// irradiating bodies: 'temperature', 'radius', 'irradiation ramp-up time' (planetary_system.cpp:160-250)
void set_irradiation(const Driver &dr, const Config &cfg)
{
    double temp[FCPT_MAX_BODIES] = {0}, rad[FCPT_MAX_BODIES] = {0}, ramp[FCPT_MAX_BODIES] = {0};
    bool any = false;
    const int n = (int)std::min<size_t>(cfg.nbody.size(), FCPT_MAX_BODIES);
    for (int k = 0; k < n; ++k) {
        const auto &b = cfg.nbody[k];
        temp[k] = b.count("temperature") ? number(dr.units, b.at("temperature"), K_TEMP) : 0.0;
        rad[k] = b.count("radius") ? number(dr.units, b.at("radius"), K_LEN) : 0.0;
        ramp[k] = b.count("irradiation ramp-up time") ? number(dr.units, b.at("irradiation ramp-up time"), K_NONE) : 0.0;
        any = any || temp[k] > 0.0;
    }
    if (any && dr.desc.eos == FCPT_EOS_IDEAL) // (without the energy equation a body's temperature heats nothing)
        CHECK(fcpt_set_body_irradiation(dr.ctx, n, temp, rad, ramp));
}

} // namespace

int main(int argc, char **argv)
{
    const Options opt = parse_command_line(argc, argv);
    Driver dr;
    const bool ranked = rank_from_environment(opt.want_ranks, dr.slab);
    dr.quiet = opt.quiet || dr.slab.rank > 0; // one voice, as logging::print_master
    dr.cfgpath = opt.cfgpath;
    Config cfg;
    if (!cfg.load(dr.cfgpath)) {
        fprintf(stderr, "Can not find config file %s!\n", dr.cfgpath.c_str());
        return 1;
    }
    config_to_desc(cfg, dr.desc, dr.units);
    dr.outdir = cfg.str("OutputDir", "output/out");
    if (dr.outdir.back() != '/')
        dr.outdir += "/";
    check_keys(cfg, opt.lenient, dr.slab.master());
    Particles pt{&dr};
    pt.ps = read_particle_setup(cfg, dr.units, dr.desc, opt.have_dust_seed, opt.want_ranks > 1 || dr.slab.nranks > 1);
    dr.sg = read_selfgravity_setup(cfg, dr.units, dr.desc, opt.want_ranks > 1 || dr.slab.nranks > 1);
    BodySystem bs{&dr};
    bs.free = opt.bodies_mode == "free";
    check_bodies_mode(cfg, dr, bs);
    if (dr.sg.on && dr.sg.indirect_disk && !(bs.free && bs.disk_feedback) && !dr.quiet)
        fprintf(stderr, "fargocpt_hip: note: IndirectTermDiskOnDisk (auto: yes with SelfGravity) is not applied: the disk's pull "
                        "on the star reaches the frame only with --bodies free and DiskFeedback: yes\n");
    // The parent of --ranks forks and execs here, unchanged: before the first library call that can open a device
    // (fcpt_device_count in create_on_device), so it has never touched a GPU.  The n ranks run, it only waits for them.
    if (opt.want_ranks > 1 && !ranked)
        return launch_ranks(opt.want_ranks, dr.outdir, dr.quiet, argv);
    const std::string restart_dir = start_mode(opt, dr);
    const bool restarting = !restart_dir.empty();
    bs.bodies = read_bodies(cfg, dr.units, dr.desc);
    GlobalFields fields = initial_fields(cfg, dr);
    std::string transport = opt.transport;
    const int ndev = create_on_device(dr, fields, transport);
    if (dr.slab.multi())
        connect_ranks(dr, transport, ndev);
    bs.init(cfg);
    bs.set(0.0);
    set_irradiation(dr, cfg);
    if (dr.sg.on)
        init_selfgravity(dr, restarting);
    CHECK(fcpt_init_physics(dr.ctx));
    pt.init();
    if (pt.ps.on && !restarting)
        pt.place_initial();
    if (dr.slab.master()) {
        mkdirs(dr.outdir + "snapshots/");
        mkdirs(dr.outdir + "monitor/");
        if (!restarting)
            write_static_files(dr);
    }
    if (!dr.quiet)
        note_unused_keys(cfg);
    calc_dt(dr); // main.cpp:117
    Run run{&dr, &bs, &pt, opt.max_steps};
    if (restarting) {
        const misc_entry misc = restart_load(dr, bs, pt, restart_dir);
        run.time = misc.time;
        run.n_monitor = misc.nTimeStep;
        run.n_iter = run.n_iter_last = misc.N_iter;
    } else if (bs.free && bs.disk_feedback) {
        bs.correct_velocity_for_disk();
    }
    exchange(dr); // CommunicateBoundariesAll, main.cpp:147
    if (!restarting) { // main.cpp:150-152, and simulation.cpp:41-47: the damping data as a reference
        write_snapshot(dr, bs, pt, 0, 0, nullptr);
        if (needs_reference(dr.desc))
            write_snapshot(dr, bs, pt, 0, 0, "reference");
    }
    CHECK(fcpt_apply_boundary(dr.ctx, 0.0, 0)); // sim::init (simulation.cpp:462-474)
    if (!restarting)
        calc_dt(dr);
    exchange(dr);
    run.begin(restarting, opt.dust_seed);
    run.loop();
    run.finish();
    fcpt_destroy(dr.ctx);
    fcpt_nbody_destroy(bs.nb);
    return 0;
}
