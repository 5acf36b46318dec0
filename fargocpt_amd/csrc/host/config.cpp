// fargocpt_hip -- the YAML setup, the code units and the descriptor of the library.
//
// Supported configuration keys: the ones the hot path consumes (SURVEY.md section 5 "Config /
// flags"); unit suffixes au / solMass / jupiterMass / earthMass / g/cm2 / K are understood
// for the default unit system (l0 = 1 au, m0 = 1 solMass).  A key the reference's reader does not know is
// fatal, as in the reference (src/config.cpp:134-138: a typo must not silently change the physics); --lenient
// downgrades that to a warning.  Keys the reference knows but the gas path does not consume are accepted (listed
// unless -q); features outside the path that a setup switches on (FLD, self-gravity with the Bessel kernel ...) are
// refused.  SelfGravity runs with SelfGravityMode: basic | symmetric (read_selfgravity_setup).
#include "driver.h"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <fstream>
#include <sstream>

std::string lower(std::string s)
{
    std::transform(s.begin(), s.end(), s.begin(), [](unsigned char c) { return (char)std::tolower(c); });
    return s;
}
static std::string trim(const std::string &s)
{
    const size_t a = s.find_first_not_of(" \t\r\n");
    if (a == std::string::npos)
        return "";
    const size_t b = s.find_last_not_of(" \t\r\n");
    return s.substr(a, b - a + 1);
}
static std::string unquote(std::string v)
{
    v = trim(v);
    if (v.size() >= 2 && (v.front() == '\'' || v.front() == '"') && v.back() == v.front())
        v = v.substr(1, v.size() - 2);
    return v;
}

bool Config::load(const std::string &path)
{
    std::ifstream f(path);
    if (!f)
        return false;
    std::string line;
    bool in_nbody = false;
    while (std::getline(f, line)) {
        // strip comments (a '#' preceded by whitespace or at column 0)
        for (size_t i = 0; i < line.size(); ++i)
            if (line[i] == '#' && (i == 0 || line[i - 1] == ' ' || line[i - 1] == '\t')) {
                line = line.substr(0, i);
                break;
            }
        if (trim(line).empty())
            continue;
        const bool indented = line[0] == ' ' || line[0] == '\t' || line[0] == '-';
        std::string t = trim(line);
        if (in_nbody && indented) {
            if (t[0] == '-') {
                nbody.emplace_back();
                t = trim(t.substr(1));
            }
            const size_t c = t.find(':');
            if (c != std::string::npos && !nbody.empty())
                nbody.back()[lower(trim(t.substr(0, c)))] = unquote(t.substr(c + 1));
            continue;
        }
        in_nbody = false;
        const size_t c = t.find(':');
        if (c == std::string::npos)
            continue;
        const std::string key = lower(trim(t.substr(0, c)));
        const std::string val = unquote(t.substr(c + 1));
        if (key == "nbody") {
            in_nbody = true;
            continue;
        }
        kv[key] = val;
    }
    return true;
}
std::string Config::str(const std::string &k, const std::string &def) const
{
    used[lower(k)] = true;
    auto it = kv.find(lower(k));
    return it == kv.end() ? def : it->second;
}
bool Config::flag(const std::string &k, bool def) const
{
    const std::string v = lower(str(k, def ? "yes" : "no"));
    return !v.empty() && (v[0] == 'y' || v[0] == 't' || v[0] == '1');
}

// Every top-level key the reference's own reader visits (config::cfg.get* / contains calls of src/parameters.cpp,
// src/Interpret.cpp, src/units.cpp, src/boundary_conditions/{config,damping}.cpp, src/particles, src/fld ..., lower
// case): a key outside this set is what src/config.cpp:134-138 dies on ("Unknown key(s) found in config file").
static const char *const kReferenceKeys[] = {
    "accretewithoutdiskfeedback", "adiabatic", "adiabaticindex", "alphacold", "alphahot", "alphamode",
    "artificialviscosity", "artificialviscositydissipation", "artificialviscosityfactor", "aspectratio",
    "aspectratiomode", "bitwiseexactrestarting", "bodyforcefrompotential", "cartesianparticles",
    "centerprofiledensitycorrectionfactor", "cfl", "cflmaxvar", "cicplanet", "circumbinarydecayexponent",
    "circumbinarydecaywidth", "circumbinaryring", "circumbinaryringenhancementfactor", "circumbinaryringposition",
    "circumbinaryringwidth", "compatibilitynostarsmoothing", "compatibilitysmoothingplanetloc", "constantviscosity",
    "coolingbeta", "coolingbetalocal", "coolingbetarampup", "coolingbetareference", "coolingbetaziampras2023",
    "coolingbetaziampras2023method", "coolingradiativefactor", "corotationreferencebody", "correctdiskselfgravity",
    "cps", "cvnr", "damping", "dampingenergyinner", "dampingenergyouter", "dampinginnerlimit", "dampingouterlimit",
    "dampingsurfacedensityinner", "dampingsurfacedensityouter", "dampingtimefactor", "dampingtimeradiusouter",
    "dampingvazimuthalinner", "dampingvazimuthalouter", "dampingvradialinner", "dampingvradialouter",
    "densityfactor", "disk", "diskfeedback", "diskmass", "diskradiusmassfraction", "dowrite1dfiles",
    "energycondition", "energyfilename", "equationofstate", "exponentialcellsizefactor", "featuresize", "firstdt",
    "flaringindex", "fluxlimiter", "frame", "heatingcoolingcfllimit", "heatingviscous", "heatingviscousfactor",
    "hydroframecenter", "hydrogenmassfraction", "imposeddiskdrift", "indirecttermdiskondisk", "indirecttermmode",
    "initializepurekeplerian", "initializevradialzero", "innerboundary", "innerboundaryenergy", "innerboundarysigma",
    "innerboundaryvazi", "innerboundaryvazikeplerianfactor", "innerboundaryvrad", "innerboundaryvradkeplerianfactor",
    "integrateparticles", "integrator", "kappaconst", "kappafactor", "keepdiskmassconstant", "klahrsmoothingradius",
    "l0", "logafterrealseconds", "logaftersteps", "m0", "massaccretionradius", "maximumtemperature",
    "minimumtemperature", "monitortimestep", "mu", "naz", "nbody", "nmonitor", "nrad", "nsnapshots",
    "numberofparticles", "omegaframe", "opacity", "outerboundary", "outerboundaryenergy", "outerboundarysigma",
    "outerboundaryvazi", "outerboundaryvazikeplerianfactor", "outerboundaryvrad", "outerboundaryvradkeplerianfactor",
    "outputdir", "particledensity", "particlediskgravityenabled", "particledustdiffusion", "particleeccentricity",
    "particlegasdragenabled", "particleintegrator", "particlemaximumescaperadius", "particlemaximumradius",
    "particleminimumescaperadius", "particleminimumradius", "particleradius", "particleradiusincreasefactor",
    "particlespeciesnumber", "particlesurfacedensityslope", "planetorbitdisktest", "polytropicconstant",
    "profilecutoffinner", "profilecutoffouter", "profilecutoffpointinner", "profilecutoffpointouter",
    "profilecutoffwidthinner", "profilecutoffwidthouter", "quantitiesradiuslimit", "radialspacing",
    "radialviscosityfactor", "radiativediffusion", "radiativediffusionautoomega", "radiativediffusionchecksolution",
    "radiativediffusiondumpdata", "radiativediffusioninnerboundary", "radiativediffusionmaxiterations",
    "radiativediffusionomega", "radiativediffusionouterboundary", "radiativediffusiontest1d",
    "radiativediffusiontest2d", "radiativediffusiontest2ddensity", "radiativediffusiontest2dk",
    "radiativediffusiontest2dsteps", "radiativediffusiontolerance", "randomfactor", "randomseed", "randomsigma",
    "rmax", "rmin", "rochelobeoverflow", "rofaveragingtime", "rofgamma", "rofplanet", "roframpingtime",
    "roftemperature", "rofvalue", "rofvariabletransfer", "scurvetype", "secondarydisk", "selfgravity",
    "selfgravityaspectratiochangethreshold", "selfgravitymode", "selfgravitystepsbetweenkernelupdate", "setsigma0",
    "shocktube", "sigma0", "sigmacondition", "sigmafilename", "sigmafloor", "sigmaslope", "spreadingring",
    "stabilizeviscosity", "surfacecooling", "t0", "taufactor", "taumin", "temp0", "temperature0",
    "thicknesssmoothing", "thicknesssmoothingsg", "transport", "vazimuthalconsidersquadropolemoment",
    "viscaccretmassflowtest", "viscousalpha", "viscousoutflowspeed", "writealpha", "writealphagrav",
    "writealphagravmean", "writealphareynolds", "writealphareynoldsmean", "writeaspectratio", "writeateverytimestep",
    "writedefaultvalues", "writedensity", "writediskquantities", "writedivv", "writeeccentricity",
    "writeeccentricitychange", "writeeffectivegamma", "writeenergy", "writefirstadiabaticindex", "writegastorques",
    "writekappa", "writelightcurves", "writelightcurvesradii", "writemassflow", "writemeanmolecularweight",
    "writepdv", "writepotential", "writepressure", "writeqminus", "writeqplus", "writeradialdissipation",
    "writeradialluminosity", "writescaleheight", "writesgaccelazi", "writesgaccelrad", "writesoundspeed", "writetau",
    "writetaucool", "writetemperature", "writetgravitational", "writetoomre", "writetorques", "writetreynolds",
    "writevelocity", "writeverticalopticaldepth", "writeviscosity", "writevisibility",};
// Features of the reference outside the gas path of this driver: a setup that switches one on is refused, not run
// without it (out of scope).
static const char *const kRefusedWhenOn[] = {"selfgravity", "radiativediffusion", "rochelobeoverflow",
                                      "keepdiskmassconstant", "circumbinaryring", "planetorbitdisktest",
                                      "viscaccretmassflowtest"};

// "<number> [unit]" -> code units for the quantity kind
double number(const Units &un, const std::string &s, Kind kind)
{
    std::istringstream is(s);
    double v = 0;
    std::string u;
    is >> v;
    is >> u;
    u = lower(u);
    if (u.empty())
        return v;
    if (kind == K_LEN) {
        if (u == "au")
            return v * AU_CM / un.L0;
        if (u == "cm")
            return v / un.L0;
        if (u == "m")
            return v * 100.0 / un.L0;
        if (u == "solradius")
            return v * 6.957e10 / un.L0;
    } else if (kind == K_MASS) {
        if (u == "solmass")
            return v * SOLMASS_G / un.M0;
        if (u == "jupitermass")
            return v * 9.547919e-4 * SOLMASS_G / un.M0;
        if (u == "earthmass")
            return v * 3.0034893e-6 * SOLMASS_G / un.M0;
    } else if (kind == K_SIGMA) {
        if (u == "g/cm2")
            return v / (un.M0 / (un.L0 * un.L0));
    } else if (kind == K_TEMP) {
        if (u == "k")
            return v / un.TEMP0;
    } else if (kind == K_VISC) {
        if (u == "cm2/s")
            return v / (un.L0 * un.L0 / un.TIME0);
    } else if (kind == K_DENS) {
        if (u == "g/cm3")
            return v / (un.M0 / (un.L0 * un.L0 * un.L0));
    }
    fprintf(stderr, "fargocpt_hip: unit '%s' in '%s' not understood\n", u.c_str(), s.c_str());
    exit(2);
}
double num(const Config &c, const Units &u, const std::string &k, double def, Kind kind)
{
    if (!c.has(k)) {
        c.used[lower(k)] = true;
        return def;
    }
    return number(u, c.str(k, ""), kind);
}

static int bc_of(const std::string &s)
{
    const std::string v = lower(s);
    if (v == "zerogradient") return FCPT_BC_ZEROGRADIENT;
    if (v == "reference") return FCPT_BC_REFERENCE;
    if (v == "reflecting") return FCPT_BC_REFLECTING;
    if (v == "outflow") return FCPT_BC_OUTFLOW;
    if (v == "keplerian") return FCPT_BC_KEPLERIAN;
    if (v == "zeroshear") return FCPT_BC_ZEROSHEAR;
    if (v == "none") return FCPT_BC_NONE;
    fprintf(stderr, "fargocpt_hip: boundary condition '%s' is not supported\n", s.c_str());
    exit(2);
}
static int damp_of(const std::string &s) // damping.cpp:152-178
{
    switch (s.empty() ? 'n' : std::tolower(s[0])) {
    case 'r': case 'i': case 'y': return FCPT_DAMP_REFERENCE;
    case 'm': return FCPT_DAMP_MEAN;
    case 'z': return FCPT_DAMP_ZERO;
    default: return FCPT_DAMP_NONE;
    }
}

// a base unit: "l0: 30 au" / "m0: 1 solMass", or a plain number in au / solMass (units.cpp:131-160), in cgs
static double base_unit(const Config &c, const char *key, double unit_cgs, const char *unit_name)
{
    std::istringstream is(c.str(key, "1.0"));
    double v = 1.0;
    std::string u;
    is >> v >> u;
    if (!u.empty() && lower(u) != unit_name) {
        fprintf(stderr, "fargocpt_hip: %s: unit '%s' not understood (%s)\n", key, u.c_str(), unit_name);
        exit(2);
    }
    return v * unit_cgs;
}

// parameters::read + Interpret (src/parameters.cpp:520-900, src/Interpret.cpp:73-700) for the
// keys of the path.  One flat list: its order decides which refusal fires first.
void config_to_desc(const Config &c, fcpt_desc &d, Units &u)
{
    fcpt_desc_default(&d);
    {
        u.L0 = base_unit(c, "l0", AU_CM, "au");
        u.M0 = base_unit(c, "m0", SOLMASS_G, "solmass");
        u.TEMP0 = G_CGS * MU / KB * u.M0 / u.L0;
        u.TIME0 = std::sqrt(u.L0 * u.L0 * u.L0 / (G_CGS * u.M0));
        if (u.L0 != AU_CM || u.M0 != SOLMASS_G) {
            // the code-unit values of sigma_SB, c and the cgs factors of the opacity laws (constants.cpp:236-262), with
            // the expressions fcpt_desc_default uses for the default units
            const double h_cgs = 6.62607015e-27, c_cgs = 2.99792458e10;
            const double E0 = u.M0 * u.L0 * u.L0 / (u.TIME0 * u.TIME0);
            const double sigma_cgs = 2. * std::pow(M_PI, 5) * std::pow(KB, 4) / (15. * std::pow(h_cgs, 3) * std::pow(c_cgs, 2));
            d.temperature_cgs = u.TEMP0;
            d.density_cgs = u.M0 / (u.L0 * u.L0 * u.L0);
            d.opacity_cgs = u.L0 * u.L0 / u.M0;
            d.sigma_sb = sigma_cgs / (E0 / (u.L0 * u.L0 * u.TIME0 * u.TEMP0 * u.TEMP0 * u.TEMP0 * u.TEMP0));
            d.c_light = c_cgs / (u.L0 / u.TIME0);
        }
    }
    d.nr_global = (int)num(c, u, "Nrad", 64);
    d.nphi = (int)num(c, u, "Naz", 64);
    d.rmin = num(c, u, "Rmin", d.rmin, K_LEN);
    d.rmax = num(c, u, "Rmax", d.rmax, K_LEN);
    switch (std::tolower(c.str("RadialSpacing", "Arithmetic")[0])) {
    case 'l': d.radial_spacing = FCPT_SPACING_LOGARITHMIC; break;
    case 'e': d.radial_spacing = FCPT_SPACING_EXPONENTIAL; break;
    default: d.radial_spacing = FCPT_SPACING_ARITHMETIC;
    }
    d.exponential_cell_size_factor = num(c, u, "ExponentialCellSizeFactor", 1.41);
    const std::string eos = lower(c.str("EquationOfState", "Isothermal"));
    d.eos = (eos == "ideal" || eos == "adiabatic") ? FCPT_EOS_IDEAL : FCPT_EOS_ISOTHERMAL;
    d.adiabatic_index = num(c, u, "AdiabaticIndex", 7.0 / 5.0);
    if (d.eos == FCPT_EOS_IDEAL && d.adiabatic_index == 1.0)
        d.eos = FCPT_EOS_ISOTHERMAL; // Interpret.cpp:425-431
    d.mu = num(c, u, "mu", 1.0);
    d.aspect_ratio = num(c, u, "AspectRatio", 0.05);
    {
        const double t0 = num(c, u, "Temperature0", -1.0, K_TEMP); // Interpret.cpp:194-197
        if (t0 > 0.0)
            d.aspect_ratio = std::sqrt(t0 * d.Rgas / d.mu);
    }
    d.flaring_index = num(c, u, "FlaringIndex", 0.0);
    { // cps: cells per scale height overwrite Nrad and Naz (Interpret.cpp:206-228)
        const double cps = num(c, u, "cps", -1.0), H = d.aspect_ratio;
        if (cps > 0) {
            if (d.radial_spacing == FCPT_SPACING_ARITHMETIC) {
                d.nr_global = (int)std::round(cps * (d.rmax - d.rmin) / H);
                d.nphi = (int)std::round(2 * M_PI / (d.rmax - d.rmin) * d.nr_global);
            } else if (d.radial_spacing == FCPT_SPACING_LOGARITHMIC) {
                d.nr_global = (int)std::round(std::log(d.rmax / d.rmin) / std::log(1 + H / cps));
                d.nphi = (int)std::round(2 * M_PI / (std::pow(d.rmax / d.rmin, 1.0 / (double)d.nr_global) - 1));
            } else {
                fprintf(stderr, "fargocpt_hip: Setting resolution is not supported for the selected radial grid spacing.\n");
                exit(2);
            }
        }
    }
    d.minimum_temperature = num(c, u, "MinimumTemperature", 3.0 / u.TEMP0, K_TEMP);
    d.maximum_temperature = num(c, u, "MaximumTemperature", 1.0e300 / u.TEMP0, K_TEMP);
    d.sigma0 = num(c, u, "Sigma0", 173.0 / (u.M0 / (u.L0 * u.L0)), K_SIGMA);
    d.sigma_slope = num(c, u, "SigmaSlope", 0.0);
    d.sigma_floor = num(c, u, "SigmaFloor", 1e-9);
    d.set_sigma0 = c.flag("SetSigma0", false);
    d.disk_mass = num(c, u, "DiskMass", 0.01, K_MASS);
    d.viscous_alpha = num(c, u, "ViscousAlpha", 0.0);
    d.constant_viscosity = num(c, u, "ConstantViscosity", 0.0, K_VISC);
    d.radial_viscosity_factor = num(c, u, "RadialViscosityFactor", 1.0);
    d.stabilize_viscosity = (int)num(c, u, "StabilizeViscosity", 0);
    switch (std::tolower(c.str("ArtificialViscosity", "SN")[0])) {
    case 'n': d.artificial_viscosity = FCPT_ARTVISC_NONE; break;
    case 't': d.artificial_viscosity = FCPT_ARTVISC_TW; break;
    default: d.artificial_viscosity = FCPT_ARTVISC_SN;
    }
    d.artificial_viscosity_dissipation = c.flag("ArtificialViscosityDissipation", true);
    d.artificial_viscosity_factor = num(c, u, "ArtificialViscosityFactor", 1.41);
    d.heating_viscous = c.flag("HeatingViscous", true);
    d.heating_viscous_factor = num(c, u, "HeatingViscousFactor", 1.0);
    { // cooling terms (src/parameters.cpp:399-490,661-665)
        const std::string sc = lower(c.str("SurfaceCooling", "No"));
        if (sc == "thermal") {
            d.cooling_surface = 1;
        } else if (!(sc == "no" || sc == "off" || sc == "false")) {
            fprintf(stderr, "fargocpt_hip: SurfaceCooling: %s is not supported\n", sc.c_str());
            exit(2);
        }
        d.cooling_radiative_factor = num(c, u, "CoolingRadiativeFactor", 1.0);
        const std::string op = lower(c.str("Opacity", "Lin"));
        if (op == "lin") { // read_opacity_config, src/parameters.cpp:424-439
            d.opacity = FCPT_OPACITY_LIN;
        } else if (op == "bell") {
            d.opacity = FCPT_OPACITY_BELL;
        } else if (op == "constant") {
            d.opacity = FCPT_OPACITY_CONST;
        } else if (op == "simple") {
            d.opacity = FCPT_OPACITY_SIMPLE;
        } else {
            fprintf(stderr, "fargocpt_hip: Invalid choice for opacity type: %s\n", op.c_str());
            exit(2);
        }
        d.kappa_const = num(c, u, "KappaConst", 1.0);
        d.kappa_factor = num(c, u, "KappaFactor", 1.0);
        d.tau_factor = num(c, u, "TauFactor", 0.5);
        d.tau_min = num(c, u, "TauMin", 0.01);
        d.density_factor = num(c, u, "DensityFactor", std::sqrt(2.0 * M_PI));
        d.cooling_beta = c.flag("CoolingBetaLocal", false);
        d.cooling_beta_value = num(c, u, "CoolingBeta", 1.0);
        d.cooling_beta_ramp_up = num(c, u, "CoolingBetaRampUp", 0.0);
        const std::string br = lower(c.str("CoolingBetaReference", "Zero"));
        d.cooling_beta_reference = br == "reference" ? FCPT_BETAREF_REFERENCE
                                   : br == "model"   ? FCPT_BETAREF_MODEL
                                   : br == "floor"   ? FCPT_BETAREF_FLOOR
                                                     : FCPT_BETAREF_ZERO;
    }
    d.fast_transport = std::tolower(c.str("Transport", "Fast")[0]) == 'f';
    const std::string lim = lower(c.str("FluxLimiter", "VanLeer"));
    d.flux_limiter = (lim == "mc" || lim == "m") ? FCPT_LIMITER_MC : FCPT_LIMITER_VANLEER;
    d.integrator = std::tolower(c.str("Integrator", "Euler")[0]) == 'l' ? FCPT_INTEGRATOR_LEAPFROG : FCPT_INTEGRATOR_EULER;
    d.cfl = num(c, u, "CFL", 0.5);
    d.cfl_max_var = num(c, u, "CFLmaxVar", 1.1);
    d.first_dt = num(c, u, "FirstDT", 1e-9);
    d.heating_cooling_cfl_limit = num(c, u, "HeatingCoolingCFLlimit", 10.0);
    d.monitor_timestep = num(c, u, "MonitorTimestep", 1.0);
    d.nmonitor = (int)num(c, u, "Nmonitor", 10);
    d.nsnapshots = (int)num(c, u, "Nsnapshots", 1000);
    d.omega_frame = num(c, u, "OmegaFrame", 0.0);
    d.thickness_smoothing = num(c, u, "ThicknessSmoothing", 0.6);
    d.body_force_from_potential = c.flag("BodyForceFromPotential", true);
    d.initialize_vradial_zero = c.flag("InitializeVradialZero", false);
    d.initialize_pure_keplerian = c.flag("InitializePureKeplerian", false);
    if ((int)num(c, u, "ShockTube", 0) == 1) {
        d.ic = FCPT_IC_SHOCKTUBE;
        d.G = d.Rgas = 1.0; // init_shock_tube_test, src/init.cpp:507-512
    } else if (c.flag("SpreadingRing", false)) {
        d.ic = FCPT_IC_SPREADING_RING;
    }
    // boundary_conditions/config.cpp:345-440 composites, :97-343 per-variable overrides
    const char *side[2] = {"Inner", "Outer"};
    for (int s = 0; s < 2; ++s) {
        const std::string comp = lower(c.str(std::string(side[s]) + "Boundary", "individual"));
        std::string sig = "zerogradient", en = "zerogradient", vr = "zerogradient";
        if (comp == "outflow") vr = "outflow";
        else if (comp == "reflecting") vr = "reflecting";
        else if (comp == "reference") sig = en = vr = "reference";
        else if (comp != "zerogradient" && comp != "individual") {
            fprintf(stderr, "fargocpt_hip: %sBoundary: %s is not supported\n", side[s], comp.c_str());
            exit(2);
        }
        d.bc_sigma[s] = bc_of(c.str(std::string(side[s]) + "BoundarySigma", sig));
        d.bc_energy[s] = bc_of(c.str(std::string(side[s]) + "BoundaryEnergy", en));
        d.bc_vrad[s] = bc_of(c.str(std::string(side[s]) + "BoundaryVrad", vr));
        d.bc_vaz[s] = bc_of(c.str(std::string(side[s]) + "BoundaryVazi", "keplerian"));
        d.keplerian_vaz_factor[s] = num(c, u, std::string(side[s]) + "BoundaryVaziKeplerianFactor", 1.0);
        d.keplerian_vrad_factor[s] = num(c, u, std::string(side[s]) + "BoundaryVradKeplerianFactor", 0.1);
        d.damp_vrad[s] = damp_of(c.str(std::string("DampingVRadial") + side[s], "None"));
        d.damp_vaz[s] = damp_of(c.str(std::string("DampingVAzimuthal") + side[s], "None"));
        d.damp_sigma[s] = damp_of(c.str(std::string("DampingSurfaceDensity") + side[s], "None"));
        d.damp_energy[s] = damp_of(c.str(std::string("DampingEnergy") + side[s], "None"));
    }
    d.profile_cutoff_outer = c.flag("ProfileCutoffOuter", false) ? 1 : 0; // parameters.cpp:762-776
    d.profile_cutoff_point_outer = num(c, u, "ProfileCutoffPointOuter", 1.0e300, K_LEN);
    d.profile_cutoff_width_outer = num(c, u, "ProfileCutoffWidthOuter", 1.0, K_LEN);
    d.profile_cutoff_inner = c.flag("ProfileCutoffInner", false) ? 1 : 0;
    d.profile_cutoff_point_inner = num(c, u, "ProfileCutoffPointInner", 0.0, K_LEN);
    d.profile_cutoff_width_inner = num(c, u, "ProfileCutoffWidthInner", 1.0, K_LEN);
    d.damping = c.flag("Damping", false);
    d.damping_inner_limit = num(c, u, "DampingInnerLimit", 1.05);
    d.damping_outer_limit = num(c, u, "DampingOuterLimit", 0.95);
    d.damping_time_factor = num(c, u, "DampingTimeFactor", 1.0);
    d.damping_time_radius_outer = num(c, u, "DampingTimeRadiusOuter", d.rmax, K_LEN);
    d.write_massflow = c.flag("WriteMassFlow", false) ? 1 : 0; // parameters.cpp:345
    // hydro centre = the first body (HydroFrameCenter: primary)
    if (!c.nbody.empty() && c.nbody[0].count("mass"))
        d.hydro_center_mass = number(u, c.nbody[0].at("mass"), K_MASS);
}

// config::Config::exit_on_unknown_key (src/config.cpp:119-138, called at src/main.cpp:111-113), then the features of the
// reference outside the gas path
void check_keys(const Config &c, bool lenient, bool master)
{
    std::string unknown;
    for (auto &kv : c.kv) {
        bool known = false;
        for (const char *k : kReferenceKeys)
            known = known || kv.first == k;
        if (!known)
            unknown += (unknown.empty() ? "" : ", ") + kv.first;
    }
    if (!unknown.empty() && master) {
        fprintf(stderr, "%sUnknown key(s) found in config file: '%s'\nMaybe there is a typo?\n",
                lenient ? "fargocpt_hip: warning: " : "", unknown.c_str());
    }
    if (!unknown.empty() && !lenient)
        exit(1);
    for (const char *k : kRefusedWhenOn)
        if (c.has(k) && c.flag(k, false)) {
            // SelfGravity with SelfGravityMode written out is read_selfgravity_setup's: it runs basic and symmetric and
            // refuses the rest by name.  Without the key the reference's default is the Bessel kernel: refused here
            if (!strcmp(k, "selfgravity") && c.has("SelfGravityMode"))
                continue;
            fprintf(stderr, "fargocpt_hip: '%s' is switched on, but that part of the reference is outside this driver's "
                            "gas path\n", k);
            exit(2);
        }
}

// keys the reference knows and this driver's gas path does not consume
void note_unused_keys(const Config &c)
{
    for (auto &kv : c.kv)
        if (!c.used.count(kv.first) && kv.first.compare(0, 5, "write") != 0 && kv.first.compare(0, 8, "particle") != 0)
            fprintf(stderr, "fargocpt_hip: note: key '%s' is not used by the gas path\n", kv.first.c_str());
}

[[noreturn]] static void refuse_particles(const char *what, bool seed_hint = false)
{
    fprintf(stderr, "fargocpt_hip: %s is not supported with IntegrateParticles\n", what);
    if (seed_hint)
        fputs("fargocpt_hip: (ParticleDustDiffusion: yes runs with --dust-seed N, the seed of its random kicks"
              "; ParticleGasDragEnabled: no only together with it)\n", stderr);
    exit(2);
}

// IntegrateParticles: the Particle* keys (parameters.cpp:853-961); what the particle step of the library does not
// cover is refused here, each with the key that asks for it, before any device is asked for
ParticleSetup read_particle_setup(const Config &c, const Units &u, const fcpt_desc &d, bool have_dust_seed, bool several_ranks)
{
    ParticleSetup ps;
    ps.on = c.flag("IntegrateParticles", false);
    ps.calculate_disk = !ps.on || c.flag("Disk", true); // without particles as before
    if (!ps.on)
        return ps;
    if (std::tolower(c.str("ParticleIntegrator", "m")[0]) != 'm')
        refuse_particles("ParticleIntegrator other than midpoint (the explicit adaptive integrator)");
    // dust diffusion is a stochastic run: it needs --dust-seed, there is no hidden default.  The drag may be
    // switched off only together with it (the reference's dust_diffusion test).
    ps.diffusion = c.flag("ParticleDustDiffusion", false);
    ps.gas_drag = c.flag("ParticleGasDragEnabled", true);
    if (!ps.gas_drag && !(ps.diffusion && have_dust_seed))
        refuse_particles("ParticleGasDragEnabled: no", true);
    if (ps.diffusion && !have_dust_seed)
        refuse_particles("ParticleDustDiffusion", true);
    if (c.flag("ParticleDiskGravityEnabled", false))
        refuse_particles("ParticleDiskGravityEnabled");
    if (lower(c.str("ParticleSurfaceDensitySlope", "SigmaSlope")) == "gas")
        refuse_particles("ParticleSurfaceDensitySlope: gas");
    if (d.integrator != FCPT_INTEGRATOR_EULER)
        refuse_particles("Integrator: Leapfrog");
    if (several_ranks)
        refuse_particles("--ranks > 1 (particles need the whole grid in one slab)");
    ps.cartesian_gravity = c.flag("CartesianParticles", false); // with the midpoint integrator: the form of the gravity only (parameters.cpp:927-932)
    ps.n = (long)num(c, u, "NumberOfParticles", 0);
    ps.radius = num(c, u, "ParticleRadius", 100.0 / u.L0, K_LEN);
    ps.species = std::max(1, (int)num(c, u, "ParticleSpeciesNumber", 1));
    ps.radius_factor = num(c, u, "ParticleRadiusIncreaseFactor", 10.0);
    ps.eccentricity = num(c, u, "ParticleEccentricity", 0.0);
    ps.density = num(c, u, "ParticleDensity", 2.65 / (u.M0 / (u.L0 * u.L0 * u.L0)), K_DENS);
    {
        const std::string sl = c.str("ParticleSurfaceDensitySlope", "SigmaSlope");
        const double slope = lower(sl) == "sigmaslope" ? d.sigma_slope : number(u, sl, K_NONE);
        ps.slope = -slope + 1.0; // r^-slope like the gas, and a factor r for the ring (parameters.cpp:875-883)
    }
    ps.rmin = num(c, u, "ParticleMinimumRadius", d.rmin, K_LEN);
    ps.rmax = num(c, u, "ParticleMaximumRadius", d.rmax, K_LEN);
    ps.escape_min = std::max(num(c, u, "ParticleMinimumEscapeRadius", d.rmin, K_LEN), d.rmin); // clamped to the grid (:943-955)
    ps.escape_max = std::min(num(c, u, "ParticleMaximumEscapeRadius", d.rmax, K_LEN), d.rmax);
    return ps;
}

[[noreturn]] static void refuse_selfgravity(const char *what)
{
    fprintf(stderr, "fargocpt_hip: %s is not supported with SelfGravity\n", what);
    exit(2);
}

// SelfGravity: yes with SelfGravityMode: basic | symmetric (parameters.cpp:698-728); what the library's solver does not
// cover is refused here, each with the key that asks for it, before any device is asked for
SelfGravitySetup read_selfgravity_setup(const Config &c, const Units &u, const fcpt_desc &d, bool several_ranks)
{
    SelfGravitySetup sg;
    if (!(c.has("SelfGravity") && c.flag("SelfGravity", false)))
        return sg;
    sg.on = true;
    const std::string mode = lower(c.str("SelfGravityMode", "besselkernel"));
    if (mode == "basic")
        sg.mode = FCPT_SG_BASIC;
    else if (mode == "symmetric")
        sg.mode = FCPT_SG_SYMMETRIC;
    else if (mode == "besselkernel")
        refuse_selfgravity("SelfGravityMode: besselkernel (it rescales the scale height by Toomre's Q inside the source step; "
                           "basic and symmetric run)");
    else {
        fprintf(stderr, "fargocpt_hip: SelfGravityMode: %s is not supported. Choices: basic, symmetric\n", mode.c_str());
        exit(2);
    }
    if (d.eos == FCPT_EOS_IDEAL)
        refuse_selfgravity("EquationOfState: ideal (the kernel's refresh from the mass-averaged aspect ratio is not built)");
    if (d.radial_spacing != FCPT_SPACING_LOGARITHMIC)
        refuse_selfgravity("RadialSpacing other than Logarithmic (the polar method needs a logarithmic grid)");
    if (several_ranks)
        refuse_selfgravity("--ranks > 1 (the solver needs the whole grid in one slab)");
    const int lengths[2] = {d.nphi, 2 * d.nr_global};
    const char *keys[2] = {"Naz", "2 x Nrad"};
    for (int k = 0; k < 2; ++k) {
        int32_t count = 0;
        if (fcpt_selftest_fft_radices(lengths[k], nullptr, 0, &count) != FCPT_OK) {
            fprintf(stderr, "fargocpt_hip: %s = %d is not supported with SelfGravity: a transform length must be at most %d "
                            "and have no prime factor above 5\n", keys[k], lengths[k], FCPT_FFT_MAX_N);
            exit(2);
        }
    }
    sg.aspect_ratio = d.aspect_ratio;
    sg.thickness_smoothing_sg = num(c, u, "ThicknessSmoothingSG", 1.2);
    sg.write_rad = c.flag("WriteSGAccelRad", false);
    sg.write_azi = c.flag("WriteSGAccelAzi", false);
    // IndirectTermDiskOnDisk: auto = yes with self-gravity (parameters.cpp:809-817)
    const std::string it = lower(c.str("IndirectTermDiskOnDisk", "auto"));
    sg.indirect_disk = it == "auto" || c.flag("IndirectTermDiskOnDisk", true);
    return sg;
}

// the nbody list: star + planets; a setup without one has the hydro centre alone
std::vector<Body> read_bodies(const Config &c, const Units &u, const fcpt_desc &d)
{
    std::vector<Body> bodies;
    for (const auto &b : c.nbody) {
        Body o;
        o.a = b.count("semi-major axis") ? number(u, b.at("semi-major axis"), K_LEN) : 0.0;
        o.m = b.count("mass") ? number(u, b.at("mass"), K_MASS) : 0.0;
        o.phase = 0.0;
        o.rsm_factor = b.count("cubic smoothing factor") ? number(u, b.at("cubic smoothing factor"), K_NONE) : 0.0;
        o.rampup = b.count("ramp-up time") ? number(u, b.at("ramp-up time"), K_NONE) : 0.0;
        o.ecc = b.count("eccentricity") ? number(u, b.at("eccentricity"), K_NONE) : 0.0;
        o.pericenter = b.count("argument of pericenter") ? number(u, b.at("argument of pericenter"), K_NONE) : 0.0;
        o.true_anomaly = b.count("trueanomaly") ? number(u, b.at("trueanomaly"), K_NONE) : 0.0;
        bodies.push_back(o);
    }
    if (bodies.empty())
        bodies.push_back(Body{0.0, d.hydro_center_mass, 0.0, 0.0, 0.0});
    return bodies;
}
