// fargocpt_hip -- the loop of sim::run (src/simulation.cpp:505-558) with handle_outputs (:50-98).
//
// Between two monitor times the loop of sim::run does nothing but step: as long as the monitor-time snapping
// cannot trigger (simulation.cpp:528-540: it needs time_left < 1.05 dt, and dt grows by at most CFLmaxVar per
// step) those steps are exactly the ones fcpt_run_steps takes with dt resident on the device -- no read-back of
// the CFL value per step, and a replayed hipGraph on the small grids of the reference's tests.  Bodies that move
// need the host every step.
#include "driver.h"

#include <algorithm>

void Run::begin(bool restarting, unsigned long long dust_seed)
{
    const ParticleSetup &ps = pt->ps;
    tlog = dr->slab.master() ? fopen((dr->outdir + "monitor/timestepLogging.dat").c_str(), restarting ? "a" : "w") : nullptr;
    if (tlog && !restarting)
        fprintf(tlog, "#version: 2\n#FargoCPT Time log for the hydro timestep size.\n"
                  "#variable: 0  | snapshot number | 1\n#variable: 1  | monitor number | 1\n"
                  "#variable: 2  | hydrostep number | 1\n#variable: 3  | Number of Hydrosteps in last monitor_timestep | 1\n"
                  "#variable: 4  | time | code\n#variable: 5  | walltime | s\n#variable: 6  | walltime per hydrostep | ms\n"
                  "#variable: 7  | mean dt | code\n#variable: 8  | min dt | code\n#variable: 9  | max dt | code\n");
    t_start = t_last = std::chrono::steady_clock::now();
    // (particles over a frozen gas -- Disk: No -- are stepped by the host-stepped loop; over a live gas around a lone star
    //  fcpt_run_steps takes their step too, with the indirect term handed to fcpt_set_bodies)
    moving = bs->bodies.size() > 1 || bs->free || (ps.on && !ps.calculate_disk);
    if (ps.on && !moving)
        CHECK(fcpt_particles_follow_run_steps(dr->ctx, 1));
    n_iter_start = n_iter;
    if (bs->free && !restarting)
        bs->write_rows(0, 0, 0.0, true);
    fcpt_clock clk0;
    CHECK(fcpt_get_clock(dr->ctx, &clk0));
    last_dt = clk0.last_dt;
    CHECK(fcpt_dt_statistics(dr->ctx, nullptr, nullptr, 1));
    if (ps.on && (ps.diffusion || !ps.gas_drag)) {
        // One particle step per hydro iteration: the generator's counter is the iteration count, set here -- after the
        // zero-length step of the initial Stokes numbers, and from misc.bin on a restart -- so that a run continued from
        // a snapshot with the same seed draws the same deviates.
        const fcpt_particle_diffusion pd = {ps.gas_drag ? 1 : 0, ps.diffusion ? 1 : 0, (uint64_t)dust_seed, (uint64_t)n_iter};
        CHECK(fcpt_particles_diffusion(dr->ctx, &pd));
    }
}

// As many steps inside fcpt_run_steps as surely end before the next monitor time; false if that is too few to pay
bool Run::device_stretch()
{
    const fcpt_desc &d = dr->desc;
    const double left = (n_monitor + 1) * d.monitor_timestep - time;
    long k = 0;
    double used = 0.0, dtj = last_dt;
    for (; k < 100000; ++k) { // worst case: every step grows by CFLmaxVar
        dtj *= d.cfl_max_var;
        if (!(left - used >= 1.05 * dtj * (1.0 + 1e-9)))
            break;
        used += dtj;
    }
    k -= 1; // one step of margin
    if (max_steps >= 0)
        k = std::min<long>(k, max_steps - (long)n_iter);
    // (without particles a stretch is taken from eight steps on, where the captured graph can be replayed, as
    //  before.  With particles from two on.  That threshold is not measured: it is set so that setups with few
    //  steps per monitor interval -- tests/golden/setups/dust_drift_live_small.yml takes six -- reach the device
    //  loop at all; a short stretch saves the read-backs of its steps, costs one fcpt_get_clock and never
    //  replays a graph)
    if (k < (pt->ps.on ? 2 : 8))
        return false;
    int64_t done = 0;
    CHECK(fcpt_run_steps(dr->ctx, k, 0, &done));
    fcpt_clock clk;
    CHECK(fcpt_get_clock(dr->ctx, &clk));
    sum_dt += clk.time - time;
    time = clk.time;
    last_dt = clk.last_dt;
    n_iter += (unsigned long)done;
    n_in_run_steps += (unsigned long)done;
    return true;
}

// One step with the host in it: bodies, particles, gas, and the monitor row when the step ends on a monitor time
void Run::host_step()
{
    const fcpt_desc &d = dr->desc;
    fcpt_ctx *ctx = dr->ctx;
    if (bs->free)
        bs->queue_disk_force(); // on the state at the start of the step; the wait of the CFL value covers it
    const double cfl_dt = calc_dt(*dr);
    last_dt = cfl_dt;
    double step_dt;
    CHECK(fcpt_snap_to_monitor(ctx, cfl_dt, &step_dt));
    const double time_next_monitor = (n_monitor + 1) * d.monitor_timestep;
    if (bs->free) {
        double ax[FCPT_MAX_BODIES], ay[FCPT_MAX_BODIES];
        bs->collect_disk_force(ax, ay);
        bs->set_free(time, step_dt, ax, ay);
    } else if (moving) {
        bs->set_circular(time, step_dt);
    }
    if (pt->ps.on) // simulation.cpp:177-180 and the particles' part of handle_corotation (:184)
        CHECK(fcpt_particles_step(ctx, step_dt, bs->itx, bs->ity, d.omega_frame * step_dt));
    if (pt->ps.calculate_disk)
        CHECK(fcpt_step(ctx, step_dt));
    if (bs->free)
        bs->advance(step_dt); // on the host, under the step's kernels
    if (pt->ps.calculate_disk) {
        exchange(*dr); // simulation.cpp:236
        CHECK(fcpt_post(ctx, step_dt));
    } else { // Disk: No -- the gas is frozen, the clock runs (simulation.cpp:226-227)
        fcpt_clock clk;
        CHECK(fcpt_get_clock(ctx, &clk));
        clk.time += step_dt;
        clk.n_hydro_iter += 1;
        CHECK(fcpt_set_clock(ctx, &clk));
    }
    time += step_dt;
    ++n_iter;
    sum_dt += step_dt;
    if (std::fabs(time_next_monitor - time) < 1e-6 * cfl_dt)
        at_monitor();
}

// A monitor time is reached: the clock's counters, the row of the time log, the bodies' rows and, every Nmonitor
// rows, a snapshot (handle_outputs, simulation.cpp:50-66)
void Run::at_monitor()
{
    const fcpt_desc &d = dr->desc;
    ++n_monitor;
    fcpt_clock clk;
    CHECK(fcpt_get_clock(dr->ctx, &clk));
    clk.n_monitor = n_monitor;
    clk.n_snapshot = n_monitor / (unsigned)d.nmonitor;
    CHECK(fcpt_set_clock(dr->ctx, &clk));
    const auto now = std::chrono::steady_clock::now();
    const double wall = std::chrono::duration<double>(now - t_start).count();
    const unsigned long nint = n_iter - n_iter_last;
    CHECK(fcpt_dt_statistics(dr->ctx, &min_dt, &max_dt, 1)); // hydro_dt_logger: kept next to the device clock
    const double ms = nint ? 1e3 * std::chrono::duration<double>(now - t_last).count() / nint : 0.0;
    if (tlog) {
        fprintf(tlog, "%u\t%u\t%lu\t%lu\t%#.16e\t%#.16e\t%#.16e\t%#.16e\t%#.16e\t%#.16e\n", clk.n_snapshot,
                n_monitor, n_iter, nint, time, wall, ms, nint ? sum_dt / nint : 0.0, min_dt, max_dt);
        fflush(tlog);
    }
    t_last = now;
    n_iter_last = n_iter;
    sum_dt = 0;
    min_dt = 1e300;
    max_dt = 0;
    if (bs->free)
        bs->write_rows(clk.n_snapshot, n_monitor, time, false);
    if (n_monitor % (unsigned)d.nmonitor == 0)
        write_snapshot(*dr, *bs, *pt, n_monitor / (unsigned)d.nmonitor, n_monitor, nullptr);
}

void Run::loop()
{
    const double t_final = (double)dr->desc.nsnapshots * dr->desc.nmonitor * dr->desc.monitor_timestep;
    while (time < t_final) {
        if (max_steps >= 0 && (long)n_iter >= max_steps)
            break;
        if (!moving && last_dt > 0.0 && device_stretch())
            continue;
        host_step();
    }
}

void Run::finish()
{
    if (tlog)
        fclose(tlog);
    CHECK(fcpt_synchronize(dr->ctx));
    barrier(*dr); // no slab tears its communicator down while another still waits in it
    const double wall = std::chrono::duration<double>(std::chrono::steady_clock::now() - t_start).count();
    if (!dr->quiet)
        printf("-- Final: Total Hydrosteps %lu, Time %.2f, Walltime %.2f seconds, Time per Step: %.2f milliseconds\n", n_iter,
               time, wall, n_iter ? 1e3 * wall / n_iter : 0.0);
    if (!dr->quiet && pt->ps.on)
        printf("-- Particles: %lu of this run's %lu hydro steps ran inside fcpt_run_steps\n", n_in_run_steps, n_iter - n_iter_start);
}
