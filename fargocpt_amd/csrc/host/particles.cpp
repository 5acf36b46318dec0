// fargocpt_hip -- dust particles with gas drag (fcpt_particles_*): placement, the library's six columns against the
// reference's record, snapshots/<n>/particles.dat and the restart from it; see DESIGN.md section 4.
// init_dust_profile / insert_particle (particles/particles.cpp:426-475,477-520)
#include "driver.h"

#include <cstring>

namespace {
// the driver's own generator for the initial placement (splitmix64; the reference's random stream is not reproduced)
struct Random {
    uint64_t state;
    double uniform() // [0, 1)
    {
        uint64_t z = (state += 0x9e3779b97f4a7c15ull);
        z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
        z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
        z ^= z >> 31;
        return (double)(z >> 11) * (1.0 / 9007199254740992.0);
    }
};
// what fcpt_particles_set / _get move: ids and r, phi, r_dot, phi_dot, radius, stokes
struct Columns {
    std::vector<uint64_t> id;
    std::vector<double> a[6];
    explicit Columns(size_t n) : id(n)
    {
        for (auto &v : a)
            v.resize(n);
    }
};
} // namespace

void Particles::init()
{
    const fcpt_desc &d = dr->desc;
    const Units &u = dr->units;
    CHECK(fcpt_particle_params_default(&d, &prm));
    if (!ps.on)
        return;
    prm.particle_density = ps.density;
    prm.molecule_mass = d.mu * MU / u.M0;
    prm.molecule_radius = 1.5e-8 / u.L0;
    prm.k_B = KB / ((u.M0 * u.L0 * u.L0 / (u.TIME0 * u.TIME0)) / u.TEMP0);
    prm.escape_radius_min = ps.escape_min;
    prm.escape_radius_max = ps.escape_max;
    prm.gravity_cartesian = ps.cartesian_gravity ? 1 : 0;
}

void Particles::upload(const std::vector<ParticleRecord> &rec)
{
    const size_t n = rec.size();
    Columns c(n);
    fixed.clear();
    for (size_t k = 0; k < n; ++k) {
        c.id[k] = rec[k].id;
        c.a[0][k] = rec[k].r, c.a[1][k] = rec[k].phi, c.a[2][k] = rec[k].r_dot, c.a[3][k] = rec[k].phi_dot;
        c.a[4][k] = rec[k].radius, c.a[5][k] = rec[k].stokes;
        fixed[rec[k].id] = {rec[k].mass, rec[k].r_ddot, rec[k].phi_ddot};
    }
    CHECK(fcpt_particles_set(dr->ctx, &prm, (int64_t)n, c.id.data(), c.a[0].data(), c.a[1].data(), c.a[2].data(), c.a[3].data(),
                             c.a[4].data(), c.a[5].data()));
}

std::vector<ParticleRecord> Particles::download()
{
    int64_t n = 0;
    CHECK(fcpt_particles_count(dr->ctx, &n));
    Columns c((size_t)n);
    CHECK(fcpt_particles_get(dr->ctx, n, c.id.data(), c.a[0].data(), c.a[1].data(), c.a[2].data(), c.a[3].data(), c.a[4].data(),
                             c.a[5].data(), &n));
    std::vector<ParticleRecord> rec((size_t)n);
    for (size_t k = 0; k < (size_t)n; ++k) {
        const std::array<double, 3> &fx = fixed[c.id[k]];
        rec[k] = ParticleRecord{c.id[k], c.a[0][k], c.a[1][k], c.a[2][k], c.a[3][k], fx[1], fx[2], fx[0], c.a[4][k], 0.0, 0.0, c.a[5][k]};
    }
    return rec;
}

void Particles::place_initial()
{
    const fcpt_desc &d = dr->desc;
    // power_law_distribution (:55-82): keep eccentric orbits inside the particle bounds
    double rmin = ps.rmin, rmax = ps.rmax;
    if (d.rmax < ps.rmax * (1.0 + ps.eccentricity))
        rmax = ps.rmax / (1.0 + ps.eccentricity);
    if (d.rmin > ps.rmin * (1.0 - ps.eccentricity))
        rmin = ps.rmin / (1.0 - ps.eccentricity);
    Random rnd{20240611ull};
    std::vector<ParticleRecord> rec((size_t)ps.n);
    for (long i = 0; i < ps.n; ++i) {
        const double x = rnd.uniform(), n1 = ps.slope + 1.0;
        const double a = ps.slope == -1.0 ? std::exp(std::log(rmax / rmin) * x) * rmin
                                          : std::exp(std::log(x * (-std::pow(rmin, n1) + std::pow(rmax, n1)) + std::pow(rmin, n1)) / n1);
        const double phi = 2.0 * M_PI * rnd.uniform();
        const double e = ps.eccentricity * rnd.uniform();
        ParticleRecord &q = rec[(size_t)i];
        memset(&q, 0, sizeof(q));
        q.id = (uint64_t)i;
        q.radius = ps.radius * std::pow(ps.radius_factor, (double)(i % ps.species));
        q.mass = 4.0 / 3.0 * M_PI * std::pow(q.radius, 3) * ps.density;
        const double r = a * (1.0 + e);
        const double v = std::sqrt(d.G * (d.hydro_center_mass + q.mass) / a) * std::sqrt((1.0 - e) / (1.0 + e));
        q.r = r;
        q.phi = phi;
        q.r_dot = 0.0;
        q.phi_dot = v / r;
        q.r_ddot = v;
        q.phi_ddot = e;
        q.stokes = 1.0;
    }
    // check_tstop (:1277-1311): the Stokes number of every particle where and as it starts.  A step of length zero of
    // the library's kernel evaluates exactly that -- the drag law at (r, phi) with the particle's own velocity -- and
    // moves nothing; its Stokes numbers go into the initial state.
    upload(rec);
    CHECK(fcpt_particles_step(dr->ctx, 0.0, 0.0, 0.0, 0.0));
    std::map<uint64_t, double> st;
    for (const ParticleRecord &q : download())
        st[q.id] = q.stokes;
    for (ParticleRecord &q : rec)
        q.stokes = st.count(q.id) ? st[q.id] : 0.0;
    upload(rec);
}

// particles::write (particles.cpp:2270-2330): the live particles, one record each
void Particles::write(const std::string &dir)
{
    const std::vector<ParticleRecord> rec = download();
    FILE *f = open_or_die(dir + "particles.dat", "wb");
    if (fwrite(rec.data(), sizeof(ParticleRecord), rec.size(), f) != rec.size())
        die_cannot("write", dir + "particles.dat");
    fclose(f);
}

// particles::restart (particles.cpp:790-890)
void Particles::read(const std::string &dir)
{
    FILE *f = open_or_die(dir + "particles.dat", "rb");
    std::vector<ParticleRecord> rec;
    ParticleRecord q;
    while (fread(&q, sizeof(q), 1, f) == 1)
        rec.push_back(q);
    fclose(f);
    upload(rec);
}
