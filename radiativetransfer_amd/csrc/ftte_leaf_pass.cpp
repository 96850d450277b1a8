// ftte_leaf_pass.cpp -- the per-leaf updates of include/ftte.h: the ionisation equilibrium, its advance over a time step, the start-up
// equilibrium, the thermal balance, the temperature over a time step and the coupled step.  One function, leaf_pass, runs an update
// from its preconditions to its results in the context; an update says what it has of its own (LeafUpdate, a check of its
// arguments, its fields of the launch record with the launch, its commit).  The records and the kernels' side are ftte_leaf.h.
// ensure_level and hydrogen_mass (the census the start-up equilibrium ends with; ftte_hydrogen_mass itself stays in ftte_chem.cpp)
// moved here with them, so that this unit needs of the library only fail, check_ready and the seven launches it reaches -- the six
// kernels' and the census's -- and tests/host/leaf_pass_check.cpp can run it on the CPU against a model of them.
#include "ftte_context.h"
#include "ftte_leaf.h"

using namespace ftte;

namespace ftte {

// the leaves' levels on the device: uploaded on first use after ftte_set_grid
int ensure_level(ftte_ctx *c)
{
    if (c->chem.level) return FTTE_OK;
    FTTE_HIP(c, c->chem.level.reserve((size_t)c->ncell));
    FTTE_HIP(c, hipMemcpyAsync(c->chem.level, c->leaf_level.data(), (size_t)c->ncell, hipMemcpyHostToDevice, c->stream));
    return FTTE_OK;
}

// computeMass over the leaves of HI (the medium's or a candidate's): the two totals [msun], deterministic
int hydrogen_mass(ftte_ctx *c, const double *HI_dev, double *neutral, double *total, const char *who)
{
    int rc = ensure_level(c);
    if (rc) return rc;
    FTTE_HIP(c, c->chem.mass.reserve(kMassParts));
    if (launch_hydrogen_mass(c->chem.level, HI_dev, c->gas.field(GasState::kRho), (long)c->ncell, c->n, c->box, c->chem.mass, c->stream))
        return fail(c, FTTE_ERR_NO_DEVICE, std::string(who) + ": kernel launch failed");
    double out[2];
    FTTE_HIP(c, hipMemcpyAsync(out, c->chem.mass + 2 * kMassBlocks, sizeof out, hipMemcpyDeviceToHost, c->stream));
    FTTE_HIP(c, hipStreamSynchronize(c->stream));
    *neutral = out[0];
    *total = out[1];
    return FTTE_OK;
}

} // namespace ftte

namespace {

// The rates of the moment as the entry points take them: the transfer's J (on the host or the device) with its table of integrals
// -- ksi for the chemistry, gamma for the heating -- or the uniform background, with or without the point sources' rates
struct LeafRates {
    int run_uvb; const double *J; bool J_on_device;
    const double *table; const char *table_name; // (the name: in the refusal)
    const double *uniform; double threshold; int use_point_rates;
};

// What an update has of its own, beside its arguments
struct LeafUpdate {
    const char *who;    // the entry point, in front of every text
    const char *stops;  // where the update stops at a leaf; the state is left as it was
    bool cooling;       // it reads the cooling table
    int planes, words;  // of ChemState::out ([planes][ncell]) and ChemState::counters it uses
    bool subcycle_map;  // it writes ChemState::subcycles_out and commits it to ChemState::subcycles
};
constexpr int kMostWords = 8;

// are the rate arguments all there?  Allocates and uploads nothing.
int check_rates(ftte_ctx *c, const char *who, const LeafRates &A)
{
    if (A.run_uvb && (!A.J || !A.table)) return fail(c, FTTE_ERR_ARG, std::string(who) + ": the transfer-driven update needs J and " + A.table_name);
    if (!A.run_uvb && !A.uniform) return fail(c, FTTE_ERR_ARG, std::string(who) + ": the uniform-background update needs the background rates");
    if (A.use_point_rates && !c->point.rates.ready(c->ncell))
        return fail(c, FTTE_ERR_STATE, std::string(who) + ": no point-source rates (ftte_set_zero_rates / ftte_point_sources)");
    return FTTE_OK;
}

// checked rate arguments into the record's head; J goes to the device if it is not there
int place_rates(ftte_ctx *c, const LeafRates &A, LeafRec &L)
{
    const double *J = A.J;
    if (A.run_uvb && !A.J_on_device) {
        const size_t nc = (size_t)c->ncell;
        FTTE_HIP(c, c->chem.J.reserve(3 * nc));
        FTTE_HIP(c, hipMemcpyAsync(c->chem.J, J, sizeof(double) * 3 * nc, hipMemcpyHostToDevice, c->stream));
        J = c->chem.J;
    }
    L.J = A.run_uvb ? J : nullptr;
    L.rates = A.use_point_rates ? c->point.rates.packed() : nullptr;
    L.run_uvb = A.run_uvb ? 1 : 0;
    if (A.table) std::memcpy(L.table, A.table, sizeof L.table);
    if (A.uniform) std::memcpy(L.uniform, A.uniform, sizeof L.uniform);
    L.threshold = A.threshold;
    return FTTE_OK;
}

// One update over all leaves, in this order: the preconditions; check(), the update's own arguments, and the rate arguments, so
// that a bad argument allocates nothing; the uploads, the output planes and the counters (the first ~0, the others 0); the
// record's head; launch(R), which fills the update's own fields and launches; the counters back; and then either the refusal --
// the state as it was -- or commit(words), which copies the results in, with max_change and the steps.
template <typename Rec, typename Check, typename Launch, typename Commit>
int leaf_pass(ftte_ctx *c, const LeafUpdate &U, const LeafRates &A, Check check, Launch launch, Commit commit, double *max_change)
{
    int rc = check_ready(c, false);
    if (rc) return rc;
    ChemState &K = c->chem;
    GasState &G = c->gas;
    const std::string who = std::string(U.who) + ": ";
    if (!K.k) return fail(c, FTTE_ERR_STATE, who + "no rate coefficients (ftte_set_rate_coefficients)");
    if (U.cooling && !K.cool) return fail(c, FTTE_ERR_STATE, who + "no cooling coefficients (ftte_set_cooling_coefficients)");
    if (!K.temperature_set) return fail(c, FTTE_ERR_STATE, who + "no temperature (ftte_set_temperature)");
    if (!G.ready_with_density(c->ncell)) return fail(c, FTTE_ERR_STATE, who + "no medium with density (ftte_set_medium with rho)");
    if ((rc = check()) || (rc = check_rates(c, U.who, A))) return rc;
    FTTE_HIP(c, hipSetDevice(c->device));
    Rec R;
    LeafRec L;
    std::memset(&R, 0, sizeof R);
    std::memset(&L, 0, sizeof L);
    if ((rc = place_rates(c, A, L)) || (rc = ensure_level(c))) return rc;
    const size_t nc = (size_t)c->ncell, nwords = (size_t)U.words;
    FTTE_HIP(c, K.out.reserve((size_t)U.planes * nc));
    FTTE_HIP(c, K.counters.reserve(nwords));
    if (U.subcycle_map) {
        FTTE_HIP(c, K.subcycles_out.reserve(nc));
        FTTE_HIP(c, K.subcycles.reserve(nc));
    }
    unsigned long long words[kMostWords] = {~0ull};
    FTTE_HIP(c, hipMemcpyAsync(K.counters, words, sizeof(words[0]) * nwords, hipMemcpyHostToDevice, c->stream));

    L.level = K.level;
    L.rho = G.field(GasState::kRho);
    L.HI = G.field(GasState::kHI); L.HeI = G.field(GasState::kHeI); L.HeII = G.field(GasState::kHeII);
    L.ncell = c->ncell; L.n = c->n; L.nratec = K.nratec;
    L.box = c->box; L.logtem0 = K.logtem0; L.logtem9 = K.logtem9; L.dlogtem = K.dlogtem;
    L.first_bad = K.counters; L.max_change = K.counters + 1; L.steps = K.counters + 2;
    put_head(R, L);
    if (launch(R)) return fail(c, FTTE_ERR_NO_DEVICE, who + "kernel launch failed");
    FTTE_HIP(c, hipMemcpyAsync(words, K.counters, sizeof(words[0]) * nwords, hipMemcpyDeviceToHost, c->stream));
    FTTE_HIP(c, hipStreamSynchronize(c->stream));
    if (words[0] != ~0ull) return fail(c, FTTE_ERR_RATES, who + U.stops + " in cell " + std::to_string(words[0]) + " (0-based cell-array index)");
    if ((rc = commit(words))) return rc;
    FTTE_HIP(c, hipStreamSynchronize(c->stream));
    if (max_change) std::memcpy(max_change, &words[1], sizeof *max_change);
    K.steps = (long long)words[2];
    return FTTE_OK;
}

// planes p0 .. p0 + count - 1 of ChemState::out into the context's per-leaf arrays dst[]
int copy_planes(ftte_ctx *c, int p0, int count, double *const *dst)
{
    const size_t nc = (size_t)c->ncell;
    for (int f = 0; f < count; ++f)
        FTTE_HIP(c, hipMemcpyAsync(dst[f], c->chem.out + (size_t)(p0 + f) * nc, sizeof(double) * nc, hipMemcpyDeviceToDevice, c->stream));
    return FTTE_OK;
}

// the species from planes p0 .. p0 + 2 into the gas, which says so
int commit_species(ftte_ctx *c, int p0)
{
    GasState &G = c->gas;
    double *const dst[3] = {G.field(GasState::kHI), G.field(GasState::kHeI), G.field(GasState::kHeII)};
    const int rc = copy_planes(c, p0, 3, dst);
    if (!rc) G.species_changed();
    return rc;
}

// the temperature and its logarithm from planes 0 and 1
int commit_temperature(ftte_ctx *c)
{
    double *const dst[2] = {c->chem.tgas, c->chem.logtem};
    return copy_planes(c, 0, 2, dst);
}

// what the three updates of the species share: the record's fields and the commit
template <typename Check>
int species_update(ftte_ctx *c, const LeafUpdate &U, const LeafRates &A, Check check, double dt, int substeps, int passes,
                   int (*launch)(const ChemRec &, hipStream_t), double *max_change)
{
    return leaf_pass<ChemRec>(
        c, U, A, check,
        [&](ChemRec &R) -> int {
            ChemState &K = c->chem;
            const size_t nc = (size_t)c->ncell;
            R.logtem = K.logtem; R.k = K.k;
            R.HI_out = K.out; R.HeI_out = K.out + nc; R.HeII_out = K.out + 2 * nc;
            R.dt = dt; R.substeps = substeps; R.passes = passes;
            return launch(R, c->stream);
        },
        [&](const unsigned long long *) -> int { return commit_species(c, 0); }, max_change);
}

// solveRateEquations (equiSources.f90:3459-3677; it stops at :3637-3654)
int solve_rates(ftte_ctx *c, const LeafRates &A, double *max_change, const char *who)
{
    const LeafUpdate U{who, "species fraction outside [0, 1]", false, 3, 4, false};
    return species_update(c, U, A, [] { return FTTE_OK; }, 0., 0, 0, launch_rate_equations, max_change);
}

int check_step(ftte_ctx *c, const std::string &who, double dt, int substeps)
{
    if (!std::isfinite(dt) || !(dt > 0.)) return fail(c, FTTE_ERR_ARG, who + "dt_s must be finite and positive");
    if (substeps < 1 || substeps > 4096) return fail(c, FTTE_ERR_ARG, who + "substeps must lie in 1 .. 4096");
    return FTTE_OK;
}

int check_clip(ftte_ctx *c, const std::string &who, double tmin, double tmax)
{
    const bool ok = std::isfinite(tmin) && std::isfinite(tmax) && tmin > 0. && tmax > tmin;
    return ok ? FTTE_OK : fail(c, FTTE_ERR_ARG, who + "0 < tmin < tmax must be finite");
}

int check_hydro(ftte_ctx *c, const std::string &who, int use_hydro)
{
    return use_hydro && !c->chem.hydro_set ? fail(c, FTTE_ERR_STATE, who + "no hydroHeating on this grid (ftte_thermal_equilibrium)") : FTTE_OK;
}

// The species advanced over dt in `substeps` implicit steps at the same rates (chem_advance_cell; the build's own, the reference
// has no time step)
int advance_rates(ftte_ctx *c, double dt, int substeps, const LeafRates &A, double *max_change, const char *who)
{
    const LeafUpdate U{who, "species not finite or outside their element's budget, or no convergence,", false, 3, 4, false};
    return species_update(c, U, A, [&] { return check_step(c, std::string(who) + ": ", dt, substeps); }, dt, substeps, 0, launch_advance_equations,
                          max_change);
}

// ---- thermal balance (ftte_thermal_math.h; kernels: ftte_thermal.hip) -------------------------------------------------------

// the thermal record's own fields: the temperature, `planes` output planes, the cooling table, Compton's numbers, the constants
void fill_thermal(ftte_ctx *c, ThermalRec &R, int planes)
{
    ChemState &K = c->chem;
    const size_t nc = (size_t)c->ncell;
    R.tgas = K.tgas;
    R.out0 = K.out; R.out1 = K.out + nc; R.out2 = planes > 2 ? K.out + 2 * nc : nullptr;
    R.cool = K.cool;
    R.coef_stride = K.cool_node_major ? 1 : K.nratec;
    R.node_stride = K.cool_node_major ? kCoolNode : 1;
    R.comp1 = K.comp1; R.comp2 = K.comp2;
    R.K = kMath;
}

// thermalEquilibrium (equiSources.f90:3870-4042): hydroHeating per leaf stays on the device
int thermal_equilibrium(ftte_ctx *c, const LeafRates &A, double *heating, double *cooling, double *hydro_heating, const char *who)
{
    const LeafUpdate U{who, "temperature not positive and finite, or heating or cooling not finite,", true, 3, 4, false};
    return leaf_pass<ThermalRec>(
        c, U, A, [] { return FTTE_OK; },
        [&](ThermalRec &R) -> int {
            fill_thermal(c, R, 3);
            return launch_thermal_equilibrium(R, c->stream);
        },
        [&](const unsigned long long *) -> int {
            ChemState &K = c->chem;
            const size_t nc = (size_t)c->ncell, bytes = sizeof(double) * nc;
            FTTE_HIP(c, K.hydro.reserve(nc));
            FTTE_HIP(c, hipMemcpyAsync(K.hydro, K.out + 2 * nc, bytes, hipMemcpyDeviceToDevice, c->stream));
            K.hydro_set = true;
            double *dst[3] = {heating, cooling, hydro_heating};
            for (int f = 0; f < 3; ++f)
                if (dst[f]) FTTE_HIP(c, hipMemcpyAsync(dst[f], K.out + f * nc, bytes, hipMemcpyDeviceToHost, c->stream));
            return FTTE_OK;
        },
        nullptr);
}

// The temperature advanced over dt in `substeps` implicit steps (thermal_advance_cell; the build's own, the reference has no time step)
int advance_temperature(ftte_ctx *c, double dt, int substeps, double tmin, double tmax, int use_hydro, const LeafRates &A, double *max_change,
                        const char *who_)
{
    const std::string who = std::string(who_) + ": ";
    const LeafUpdate U{who_, "temperature or heat capacity not finite and positive, rates not finite, or no convergence,", true, 2, 4, false};
    return leaf_pass<ThermalRec>(
        c, U, A,
        [&]() -> int {
            int rc;
            if ((rc = check_step(c, who, dt, substeps)) || (rc = check_clip(c, who, tmin, tmax))) return rc;
            return check_hydro(c, who, use_hydro);
        },
        [&](ThermalRec &R) -> int {
            fill_thermal(c, R, 2);
            R.dt = dt; R.substeps = substeps; R.tmin = tmin; R.tmax = tmax;
            R.hydro = use_hydro ? c->chem.hydro.get() : nullptr;
            return launch_thermal_advance(R, c->stream);
        },
        [&](const unsigned long long *) -> int { return commit_temperature(c); }, max_change);
}

// Species and temperature advanced together over dt, each leaf in subcycles of its own (thermochem_advance_cell; the build's own).
// The rate arguments of the pass are the heating's (J, gamma, uniform_gamma); the chemistry's tables (ksi, uniform) are the
// update's own.  Planes 0, 1: T and its logarithm; 2..4: the species.  Words 4..7: the largest change of T, the subcycles' sum
// and maximum, the leaves the cap bounded.
int advance_thermochemistry(ftte_ctx *c, double dt, double eta, int max_subcycles, double tmin, double tmax, int use_hydro, const LeafRates &A,
                            const double *ksi, const double *uniform, double *max_change, int64_t *subcycles, const char *who_)
{
    const std::string who = std::string(who_) + ": ";
    const LeafUpdate U{who_, "species, temperature or heat capacity not finite or out of range, rates not finite, or no convergence,", true, 5, 8, true};
    return leaf_pass<ThermochemRec>(
        c, U, A,
        [&]() -> int {
            int rc;
            if (!std::isfinite(dt) || !(dt > 0.)) return fail(c, FTTE_ERR_ARG, who + "dt_s must be finite and positive");
            if (!std::isfinite(eta) || !(eta >= 0.)) return fail(c, FTTE_ERR_ARG, who + "eta must be finite and not negative");
            if (max_subcycles < 1 || max_subcycles > 4096) return fail(c, FTTE_ERR_ARG, who + "max_subcycles must lie in 1 .. 4096");
            if ((rc = check_clip(c, who, tmin, tmax))) return rc;
            if (A.run_uvb ? !ksi : !uniform) return fail(c, FTTE_ERR_ARG, who + (A.run_uvb ? "the transfer-driven update needs ksi" : "the uniform-background update needs the background rates"));
            return check_hydro(c, who, use_hydro);
        },
        [&](ThermochemRec &W) -> int {
            ChemState &K = c->chem;
            const size_t nc = (size_t)c->ncell;
            fill_thermal(c, W.T, 2);
            W.T.dt = dt; W.T.tmin = tmin; W.T.tmax = tmax; W.T.substeps = 1;
            W.T.hydro = use_hydro ? K.hydro.get() : nullptr;
            W.logtem = K.logtem; W.k = K.k;
            W.HI_out = K.out + 2 * nc; W.HeI_out = K.out + 3 * nc; W.HeII_out = K.out + 4 * nc;
            W.subcycles = K.subcycles_out;
            if (ksi) std::memcpy(W.ksi, ksi, sizeof W.ksi);
            if (uniform) std::memcpy(W.uniform, uniform, sizeof W.uniform);
            W.eta = eta; W.max_subcycles = max_subcycles;
            W.max_tchange = K.counters + 4; W.sub_sum = K.counters + 5; W.sub_max = K.counters + 6; W.capped = K.counters + 7;
            return launch_thermochem_advance(W, c->stream);
        },
        [&](const unsigned long long *words) -> int {
            ChemState &K = c->chem;
            int rc;
            if ((rc = commit_species(c, 2)) || (rc = commit_temperature(c))) return rc;
            FTTE_HIP(c, hipMemcpyAsync(K.subcycles, K.subcycles_out, sizeof(int32_t) * (size_t)c->ncell, hipMemcpyDeviceToDevice, c->stream));
            K.subcycles_set = true;
            if (max_change) std::memcpy(&max_change[1], &words[4], sizeof(double));
            if (subcycles) for (int i = 0; i < 3; ++i) subcycles[i] = (int64_t)words[5 + i];
            return FTTE_OK;
        },
        max_change);
}

} // namespace

extern "C" {

int ftte_thermal_equilibrium(ftte_ctx *c, int run_uvb_transfer, const double *J, const double *gamma, const double *uniform_gamma,
                             double self_shielding_threshold, int use_point_rates, double *heating, double *cooling, double *hydro_heating)
{
    const LeafRates A{run_uvb_transfer, J, false, gamma, "gamma", uniform_gamma, self_shielding_threshold, use_point_rates};
    return thermal_equilibrium(c, A, heating, cooling, hydro_heating, "ftte_thermal_equilibrium");
}

int ftte_thermal_equilibrium_device(ftte_ctx *c, int run_uvb_transfer, const double *J_dev, const double *gamma, const double *uniform_gamma,
                                    double self_shielding_threshold, int use_point_rates, double *heating, double *cooling,
                                    double *hydro_heating)
{
    const LeafRates A{run_uvb_transfer, J_dev, true, gamma, "gamma", uniform_gamma, self_shielding_threshold, use_point_rates};
    return thermal_equilibrium(c, A, heating, cooling, hydro_heating, "ftte_thermal_equilibrium_device");
}

int ftte_advance_temperature(ftte_ctx *c, double dt_s, int substeps, double tmin, double tmax, int use_hydro_heating, int run_uvb_transfer,
                             const double *J, const double *gamma, const double *uniform_gamma, double self_shielding_threshold,
                             int use_point_rates, double *max_change)
{
    const LeafRates A{run_uvb_transfer, J, false, gamma, "gamma", uniform_gamma, self_shielding_threshold, use_point_rates};
    return advance_temperature(c, dt_s, substeps, tmin, tmax, use_hydro_heating, A, max_change, "ftte_advance_temperature");
}

int ftte_advance_temperature_device(ftte_ctx *c, double dt_s, int substeps, double tmin, double tmax, int use_hydro_heating,
                                    int run_uvb_transfer, const double *J_dev, const double *gamma, const double *uniform_gamma,
                                    double self_shielding_threshold, int use_point_rates, double *max_change)
{
    const LeafRates A{run_uvb_transfer, J_dev, true, gamma, "gamma", uniform_gamma, self_shielding_threshold, use_point_rates};
    return advance_temperature(c, dt_s, substeps, tmin, tmax, use_hydro_heating, A, max_change, "ftte_advance_temperature_device");
}

int ftte_advance_thermochemistry(ftte_ctx *c, double dt_s, double eta, int max_subcycles, double tmin, double tmax, int use_hydro_heating,
                                 int run_uvb_transfer, const double *J, const double *ksi, const double *gamma, const double *uniform,
                                 const double *uniform_gamma, double self_shielding_threshold, int use_point_rates, double *max_change,
                                 int64_t *subcycles)
{
    const LeafRates A{run_uvb_transfer, J, false, gamma, "gamma", uniform_gamma, self_shielding_threshold, use_point_rates};
    return advance_thermochemistry(c, dt_s, eta, max_subcycles, tmin, tmax, use_hydro_heating, A, ksi, uniform, max_change, subcycles,
                                   "ftte_advance_thermochemistry");
}

int ftte_advance_thermochemistry_device(ftte_ctx *c, double dt_s, double eta, int max_subcycles, double tmin, double tmax, int use_hydro_heating,
                                        int run_uvb_transfer, const double *J_dev, const double *ksi, const double *gamma, const double *uniform,
                                        const double *uniform_gamma, double self_shielding_threshold, int use_point_rates, double *max_change,
                                        int64_t *subcycles)
{
    const LeafRates A{run_uvb_transfer, J_dev, true, gamma, "gamma", uniform_gamma, self_shielding_threshold, use_point_rates};
    return advance_thermochemistry(c, dt_s, eta, max_subcycles, tmin, tmax, use_hydro_heating, A, ksi, uniform, max_change, subcycles,
                                   "ftte_advance_thermochemistry_device");
}

int ftte_solve_rate_equations(ftte_ctx *c, int run_uvb_transfer, const double *J, const double *ksi, const double *uniform,
                              double self_shielding_threshold, int use_point_rates, double *max_change)
{
    const LeafRates A{run_uvb_transfer, J, false, ksi, "ksi", uniform, self_shielding_threshold, use_point_rates};
    return solve_rates(c, A, max_change, "ftte_solve_rate_equations");
}

int ftte_solve_rate_equations_device(ftte_ctx *c, int run_uvb_transfer, const double *J_dev, const double *ksi, const double *uniform,
                                     double self_shielding_threshold, int use_point_rates, double *max_change)
{
    const LeafRates A{run_uvb_transfer, J_dev, true, ksi, "ksi", uniform, self_shielding_threshold, use_point_rates};
    return solve_rates(c, A, max_change, "ftte_solve_rate_equations_device");
}

int ftte_advance_rate_equations(ftte_ctx *c, double dt_s, int substeps, int run_uvb_transfer, const double *J, const double *ksi,
                                const double *uniform, double self_shielding_threshold, int use_point_rates, double *max_change)
{
    const LeafRates A{run_uvb_transfer, J, false, ksi, "ksi", uniform, self_shielding_threshold, use_point_rates};
    return advance_rates(c, dt_s, substeps, A, max_change, "ftte_advance_rate_equations");
}

int ftte_advance_rate_equations_device(ftte_ctx *c, double dt_s, int substeps, int run_uvb_transfer, const double *J_dev, const double *ksi,
                                       const double *uniform, double self_shielding_threshold, int use_point_rates, double *max_change)
{
    const LeafRates A{run_uvb_transfer, J_dev, true, ksi, "ksi", uniform, self_shielding_threshold, use_point_rates};
    return advance_rates(c, dt_s, substeps, A, max_change, "ftte_advance_rate_equations_device");
}

// initialIonizationEquilibrium (it stops at equiSources.f90:3809-3818, :3832-3843): the uniform background alone
int ftte_initial_ionization_equilibrium(ftte_ctx *c, const double *uniform, double threshold, int passes, double *neutral_fraction)
{
    const char *who = "ftte_initial_ionization_equilibrium";
    const LeafUpdate U{who, "species fraction outside [0, 1] or no convergence", false, 3, 4, false};
    const LeafRates A{0, nullptr, false, nullptr, "", uniform, threshold, 0};
    int rc = species_update(c, U, A, [&]() -> int {
        const int bad = check_rates(c, who, A); // (in front of `passes`, as ever)
        if (bad) return bad;
        return passes < 1 ? fail(c, FTTE_ERR_ARG, std::string(who) + ": passes must be at least 1") : FTTE_OK;
    }, 0., 0, passes, launch_initial_equilibrium, nullptr);
    if (rc || !neutral_fraction) return rc;
    // equiSources.f90:1020-1022
    double neutral = 0., total = 0.;
    if ((rc = hydrogen_mass(c, c->gas.field(GasState::kHI), &neutral, &total, who))) return rc;
    *neutral_fraction = neutral / total;
    return FTTE_OK;
}

long long ftte_rate_equation_steps(const ftte_ctx *c) { return c ? c->chem.steps : 0; }

} // extern "C"
