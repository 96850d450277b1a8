// ftte_chem.cpp -- the entry points of include/ftte.h that read or write the species medium (ftte_ctx::gas) outside the tracer and
// outside the per-leaf updates (ftte_leaf_pass.cpp): the chemistry's tables and the temperature, the hydrogen census, the species' way
// out, the opacities and the thin-limit radiation made from them, and the start-up expansion of HII regions (kernel:
// ftte_expansion.hip).  The chemistry's own state is ftte_ctx::chem.
#include <cstdlib>

#include "ftte_chem_math.h"
#include "ftte_context.h"
#include "ftte_leaf.h"
#include "ftte_thermal_math.h"

using namespace ftte;

namespace {

int assign_uvb(ftte_ctx *c, int nnu, const double *uvb, double threshold, double *J, bool J_on_device, const char *who)
{
    int rc = check_ready(c, false);
    if (rc) return rc;
    if (nnu < 1 || !uvb || !J) return fail(c, FTTE_ERR_ARG, std::string(who) + ": bad argument");
    const GasState &G = c->gas;
    if (!G.ready_with_density(c->ncell)) return fail(c, FTTE_ERR_STATE, std::string(who) + ": no medium with density (ftte_set_medium with rho)");
    FTTE_HIP(c, hipSetDevice(c->device));
    const size_t nc = (size_t)c->ncell;
    DeviceBuffer<double> duvb, J_tmp;
    FTTE_HIP(c, duvb.reserve((size_t)nnu));
    hipError_t e = hipSuccess;
    if (!J_on_device) e = J_tmp.reserve(nc * nnu);
    double *const dJ = J_on_device ? J : J_tmp.get();
    if (e == hipSuccess) e = hipMemcpyAsync(duvb, uvb, sizeof(double) * nnu, hipMemcpyHostToDevice, c->stream);
    int lrc = 0;
    if (e == hipSuccess)
        lrc = launch_thin_limit(G.field(GasState::kHI), G.field(GasState::kHeI), G.field(GasState::kHeII), G.field(GasState::kRho), duvb, threshold, dJ,
                                (long)nc, nnu, c->stream);
    if (e == hipSuccess && !J_on_device) e = hipMemcpyAsync(J, dJ, sizeof(double) * nc * nnu, hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e != hipSuccess) return fail(c, FTTE_ERR_NO_DEVICE, std::string(who) + ": " + hipGetErrorString(e));
    if (lrc) return fail(c, FTTE_ERR_NO_DEVICE, std::string(who) + ": kernel launch failed");
    return FTTE_OK;
}


// ---- expansion of HII regions (equiSources.f90:1035-1069) ------------------------------------------------------------------

// a leaf's place in the tree from its node: the child taken at every refined ancestor, the base cell at the end
LeafPos leaf_position(const AmrTree &T, int32_t node)
{
    LeafPos P;
    std::memset(&P, 0, sizeof P);
    P.depth = T.level[(size_t)node];
    int32_t at = node;
    for (int l = P.depth - 1; l >= 0; --l) {
        const int32_t up = T.parent[(size_t)at];
        P.path[l / 10] |= (uint32_t)(at - T.child0[(size_t)up]) << (3 * (l % 10));
        at = up;
    }
    P.base = at;
    return P;
}

// refined cell arrays: the leaves' position records on the device and their nodes on the host, made on first use after ftte_set_grid
int ensure_leaf_positions(ftte_ctx *c)
{
    ChemState &K = c->chem;
    if (!c->tree.refined() || (K.leaf_pos && (int64_t)K.leaf_node.size() == c->ncell)) return FTTE_OK;
    const AmrTree &T = c->tree;
    std::vector<LeafPos> pos((size_t)c->ncell);
    K.leaf_node.assign((size_t)c->ncell, -1);
    for (size_t node = 0; node < T.leaf.size(); ++node)
        if (T.leaf[node] >= 0) {
            pos[(size_t)T.leaf[node]] = leaf_position(T, (int32_t)node);
            K.leaf_node[(size_t)T.leaf[node]] = (int32_t)node;
        }
    FTTE_HIP(c, K.leaf_pos.reserve(pos.size()));
    hipError_t e = hipMemcpyAsync(K.leaf_pos, pos.data(), sizeof(LeafPos) * pos.size(), hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream); // (pos is a local)
    if (e != hipSuccess) {
        K.leaf_pos.reset();
        return fail(c, FTTE_ERR_NO_DEVICE, std::string("ftte_expand_hii_regions: ") + hipGetErrorString(e));
    }
    return FTTE_OK;
}

} // namespace

namespace ftte {

// computeExpansionParameters(nh), equiSources.f90:4395-4429.  The tables are single-precision constructors assigned to double
// arrays (:4406-4408); 10.**x has a double exponent, so it is pow(10, x) in double.
void expansion_parameters(double nh, double *final_radius_cm, double *density_coefficient)
{
    static const float LIf[10] = {0.00000f, 0.333333f, 0.666667f, 1.00000f, 1.33333f, 1.66667f, 2.00000f, 2.33333f, 2.66667f, 3.00000f};
    static const float LRf[10] = {2.99506f, 2.77808f, 2.57210f, 2.37683f, 2.19731f, 2.02898f, 1.87315f, 1.73656f, 1.61294f, 1.50202f};
    static const float LDf[10] = {-0.0222764f, 0.295050f, 0.579490f, 0.831870f, 1.03717f, 1.20892f, 1.34321f, 1.41970f, 1.45725f, 1.45667f};
    const double pc = (double)3.08568025e18f; // definitionsModule.f90:21
    double LI[10], LR[10], LD[10];
    for (int q = 0; q < 10; ++q) { LI[q] = (double)LIf[q]; LR[q] = (double)LRf[q]; LD[q] = (double)LDf[q]; }
    const double lognh = std::log10(nh);
    int i = 1; // 1-based, as the reference counts
    while (lognh > LI[i - 1] && i < 10) ++i;
    i = std::max(i, 2);
    double tmp = (lognh - LI[i - 2]) / (LI[i - 1] - LI[i - 2]);
    *final_radius_cm = std::pow(10.0, tmp * (LR[i - 1] - LR[i - 2]) + LR[i - 2]) * pc;
    *density_coefficient = std::pow(10.0, tmp * (LD[i - 1] - LD[i - 2]) + LD[i - 2]) / nh;
    if (lognh < LI[0]) {
        tmp = (lognh + 6.0) / (LI[0] + 6.0);
        *density_coefficient = std::pow(10.0, tmp * (LD[0] + 6.0) - 6.0) / nh;
    }
}

// absoluteCoordinates (equiSources.f90:3011-3047) from startingPoint = (.5, .5, .5): from the leaf upwards the point is halved
// (child 1) or halved and moved by a half (child 2), then (float(i-1) + p) / float(nx)
void expansion_star_centre(const LeafPos &P, int n, double *x, double *y, double *z)
{
    double p[3] = {0.5, 0.5, 0.5};
    for (int l = P.depth - 1; l >= 0; --l) {
        const uint32_t bits = P.path[l / 10] >> (3 * (l % 10));
        for (int a = 0; a < 3; ++a) p[a] = (bits & (4u >> a)) ? 0.5 * p[a] + 0.5 : 0.5 * p[a];
    }
    const int i0[3] = {P.base / (n * n), (P.base / n) % n, P.base % n};
    double *out[3] = {x, y, z};
    for (int a = 0; a < 3; ++a) *out[a] = ((double)(float)i0[a] + p[a]) / (double)(float)n;
}

} // namespace ftte

extern "C" {

int ftte_set_rate_coefficients(ftte_ctx *c, int nratec, double logtem0, double logtem9, double dlogtem, const double *k1a,
                               const double *k2a, const double *k3a, const double *k4a, const double *k5a, const double *k6a)
{
    int rc = check_single(c);
    if (rc) return rc;
    if (nratec < 2 || !(dlogtem > 0.0) || !(logtem9 > logtem0) || !k1a || !k2a || !k3a || !k4a || !k5a || !k6a)
        return fail(c, FTTE_ERR_ARG, "ftte_set_rate_coefficients: bad argument");
    ChemState &K = c->chem;
    FTTE_HIP(c, hipSetDevice(c->device));
    FTTE_HIP(c, hipStreamSynchronize(c->stream));
    if (K.nratec != nratec) { K.k.reset(); K.cool.reset(); K.ground.reset(); } // (the cooling and the ground-state coefficients share the temperature grid)
    FTTE_HIP(c, K.k.reserve(6 * (size_t)nratec));
    const double *src[6] = {k1a, k2a, k3a, k4a, k5a, k6a};
    for (int r = 0; r < 6; ++r)
        FTTE_HIP(c, hipMemcpyAsync(K.k + (size_t)r * nratec, src[r], sizeof(double) * nratec, hipMemcpyHostToDevice, c->stream));
    FTTE_HIP(c, hipStreamSynchronize(c->stream));
    K.nratec = nratec;
    K.logtem0 = logtem0; K.logtem9 = logtem9; K.dlogtem = dlogtem;
    return FTTE_OK;
}

int ftte_set_temperature(ftte_ctx *c, const double *tgas)
{
    int rc = check_ready(c, false);
    if (rc) return rc;
    if (!tgas) return fail(c, FTTE_ERR_ARG, "ftte_set_temperature: bad argument");
    FTTE_HIP(c, hipSetDevice(c->device));
    // the logarithm is taken here, on the host, so that the device update consists of IEEE-exact operations only
    std::vector<double> logtem((size_t)c->ncell);
    {
        const int nthreads = (int)std::max(1u, std::min(16u, std::thread::hardware_concurrency()));
        const int64_t chunk = (c->ncell + nthreads - 1) / nthreads;
        std::vector<std::thread> pool;
        for (int t = 0; t < nthreads; ++t)
            pool.emplace_back([&, t] {
                const int64_t lo = t * chunk, hi = std::min<int64_t>(c->ncell, lo + chunk);
                for (int64_t q = lo; q < hi; ++q) logtem[(size_t)q] = std::log(tgas[q]);
            });
        for (auto &th : pool) th.join();
    }
    FTTE_HIP(c, c->chem.logtem.reserve((size_t)c->ncell));
    FTTE_HIP(c, hipMemcpyAsync(c->chem.logtem, logtem.data(), sizeof(double) * (size_t)c->ncell, hipMemcpyHostToDevice, c->stream));
    // the temperature itself, for the thermal balance
    FTTE_HIP(c, c->chem.tgas.reserve((size_t)c->ncell));
    FTTE_HIP(c, hipMemcpyAsync(c->chem.tgas, tgas, sizeof(double) * (size_t)c->ncell, hipMemcpyHostToDevice, c->stream));
    FTTE_HIP(c, hipStreamSynchronize(c->stream));
    c->chem.temperature_set = true;
    return FTTE_OK;
}

int ftte_get_temperature(ftte_ctx *c, double *tgas)
{
    int rc = check_ready(c, false);
    if (rc) return rc;
    if (!tgas) return fail(c, FTTE_ERR_ARG, "ftte_get_temperature: bad argument");
    if (!c->chem.temperature_set) return fail(c, FTTE_ERR_STATE, "ftte_get_temperature: no temperature (ftte_set_temperature)");
    FTTE_HIP(c, hipSetDevice(c->device));
    FTTE_HIP(c, hipMemcpyAsync(tgas, c->chem.tgas, sizeof(double) * (size_t)c->ncell, hipMemcpyDeviceToHost, c->stream));
    FTTE_HIP(c, hipStreamSynchronize(c->stream));
    return FTTE_OK;
}

int ftte_set_cooling_coefficients(ftte_ctx *c, int nratec, const double *coef, double compa, double redshift)
{
    const std::string who = "ftte_set_cooling_coefficients: ";
    int rc = check_single(c);
    if (rc) return rc;
    if (nratec < 2 || !coef || !std::isfinite(compa) || !std::isfinite(redshift)) return fail(c, FTTE_ERR_ARG, who + "bad argument");
    ChemState &K = c->chem;
    if (!K.k) return fail(c, FTTE_ERR_STATE, who + "no rate coefficients (ftte_set_rate_coefficients): the two share one temperature grid");
    if (nratec != K.nratec) return fail(c, FTTE_ERR_ARG, who + "nratec must be that of ftte_set_rate_coefficients, " + std::to_string(K.nratec));
    // The device copy: the caller's [13][nratec] as it stands.  FTTE_THERMAL_TABLE=nodes in the environment makes it node-major
    // instead -- the thirteen coefficients of a temperature node side by side, padded to 128 bytes, so that the two nodes of a
    // look-up are two adjacent cache lines and not 26 scattered words -- for measurements only: it measured 2.4 times slower
    // (the section on the thermal balance).
    const char *env = std::getenv("FTTE_THERMAL_TABLE");
    K.cool_node_major = env && !std::strcmp(env, "nodes");
    std::vector<double> table;
    if (K.cool_node_major) {
        table.assign((size_t)kCoolNode * nratec, 0.);
        for (int r = 0; r < THERMAL_NCOEF; ++r)
            for (int i = 0; i < nratec; ++i) table[(size_t)i * kCoolNode + r] = coef[(size_t)r * nratec + i];
    } else table.assign(coef, coef + (size_t)THERMAL_NCOEF * nratec);
    FTTE_HIP(c, hipSetDevice(c->device));
    FTTE_HIP(c, hipStreamSynchronize(c->stream));
    K.cool.reset();
    FTTE_HIP(c, K.cool.reserve(table.size()));
    hipError_t e = hipMemcpyAsync(K.cool, table.data(), sizeof(double) * table.size(), hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream); // (table is a local)
    if (e != hipSuccess) { K.cool.reset(); return fail(c, FTTE_ERR_NO_DEVICE, who + hipGetErrorString(e)); }
    const double a = 1. + redshift;
    K.comp1 = compa * ((a * a) * (a * a)); // compa * (1. + currentRedshift)**4, equiSources.f90:3970
    K.comp2 = FTTE_T_CMB * a;              // :3971
    return FTTE_OK;
}

int ftte_get_subcycles(ftte_ctx *c, int32_t *per_leaf)
{
    int rc = check_ready(c, false);
    if (rc) return rc;
    if (!per_leaf) return fail(c, FTTE_ERR_ARG, "ftte_get_subcycles: bad argument");
    if (!c->chem.subcycles_set) return fail(c, FTTE_ERR_STATE, "ftte_get_subcycles: no coupled step on this grid yet (ftte_advance_thermochemistry)");
    FTTE_HIP(c, hipSetDevice(c->device));
    FTTE_HIP(c, hipMemcpyAsync(per_leaf, c->chem.subcycles, sizeof(int32_t) * (size_t)c->ncell, hipMemcpyDeviceToHost, c->stream));
    FTTE_HIP(c, hipStreamSynchronize(c->stream));
    return FTTE_OK;
}

int ftte_hydrogen_mass(ftte_ctx *c, double *neutral_msun, double *total_msun)
{
    const char *who = "ftte_hydrogen_mass";
    int rc = check_ready(c, false);
    if (rc) return rc;
    if (!neutral_msun || !total_msun) return fail(c, FTTE_ERR_ARG, std::string(who) + ": bad argument");
    if (!c->gas.ready_with_density(c->ncell)) return fail(c, FTTE_ERR_STATE, std::string(who) + ": no medium with density (ftte_set_medium with rho)");
    FTTE_HIP(c, hipSetDevice(c->device));
    return hydrogen_mass(c, c->gas.field(GasState::kHI), neutral_msun, total_msun, who);
}

int ftte_get_medium(ftte_ctx *c, double *HI, double *HeI, double *HeII)
{
    int rc = check_ready(c, false);
    if (rc) return rc;
    if (!HI || !HeI || !HeII) return fail(c, FTTE_ERR_ARG, "ftte_get_medium: bad argument");
    if (!c->gas.ready(c->ncell)) return fail(c, FTTE_ERR_STATE, "no medium: call ftte_set_medium first");
    FTTE_HIP(c, hipSetDevice(c->device));
    double *dst[3] = {HI, HeI, HeII};
    for (int f = 0; f < 3; ++f)
        FTTE_HIP(c, hipMemcpyAsync(dst[f], c->gas.field(f), sizeof(double) * (size_t)c->ncell, hipMemcpyDeviceToHost, c->stream));
    FTTE_HIP(c, hipStreamSynchronize(c->stream));
    return FTTE_OK;
}

int ftte_expansion_parameters(double nh, double *final_radius_cm, double *density_coefficient)
{
    if (!final_radius_cm || !density_coefficient) return FTTE_ERR_ARG;
    expansion_parameters(nh, final_radius_cm, density_coefficient);
    return FTTE_OK;
}

int ftte_expand_hii_regions(ftte_ctx *c, int nsrc, const int64_t *src_cell, const double *params, double *rho_coef, int64_t *nchanged)
{
    const std::string who = "ftte_expand_hii_regions: ";
    int rc = check_ready(c, false);
    if (rc) return rc;
    ChemState &K = c->chem;
    GasState &G = c->gas;
    if (!G.ready_with_density(c->ncell)) return fail(c, FTTE_ERR_STATE, who + "no medium with density (ftte_set_medium with rho)");
    if (nsrc < 0 || (nsrc > 0 && !src_cell)) return fail(c, FTTE_ERR_ARG, who + "bad argument");
    for (int s = 0; s < nsrc; ++s)
        if (src_cell[s] < 0 || src_cell[s] >= c->ncell)
            return fail(c, FTTE_ERR_ARG, who + "host cell of source " + std::to_string(s) + " outside the cell array");
    const size_t nc = (size_t)c->ncell;
    if (nsrc == 0) { // no star with weight > 0: rhoCoef stays 1 everywhere
        if (rho_coef) std::fill(rho_coef, rho_coef + nc, 1.0);
        if (nchanged) *nchanged = 0;
        K.expansion_tests = 0;
        return FTTE_OK;
    }
    FTTE_HIP(c, hipSetDevice(c->device));
    if ((rc = ensure_leaf_positions(c))) return rc;
    const size_t ns = (size_t)nsrc;

    // per star: finalRadius, densityCoefficient, sourceTotalHydrogenDensity (:1048), given or from the host leaf's density
    std::vector<double> own;
    if (!params) {
        std::vector<double> rho(ns);
        FTTE_HIP(c, K.exp_cells.reserve(ns));
        FTTE_HIP(c, K.out.reserve(std::max(ns, nc)));
        FTTE_HIP(c, hipMemcpyAsync(K.exp_cells, src_cell, sizeof(int64_t) * ns, hipMemcpyHostToDevice, c->stream));
        if (launch_gather(G.field(GasState::kRho), K.exp_cells, nsrc, K.out, c->stream.get()))
            return fail(c, FTTE_ERR_NO_DEVICE, who + "kernel launch failed");
        FTTE_HIP(c, hipMemcpyAsync(rho.data(), K.out, sizeof(double) * ns, hipMemcpyDeviceToHost, c->stream));
        FTTE_HIP(c, hipStreamSynchronize(c->stream));
        own.resize(3 * ns);
        for (size_t s = 0; s < ns; ++s) {
            if (!(rho[s] > 0.0) || !std::isfinite(rho[s]))
                return fail(c, FTTE_ERR_ARG, who + "the density of the host cell of source " + std::to_string(s) + " (cell " +
                                                 std::to_string(src_cell[s]) + ") is not positive and finite");
            const double nh = chem_nh(rho[s]);
            expansion_parameters(nh, &own[3 * s], &own[3 * s + 1]);
            own[3 * s + 2] = nh;
        }
        params = own.data();
    }

    std::vector<ExpStar> star(ns);
    std::vector<ExpStarTest> test(ns);
    const double margin = (double)1.0001f; // equiSources.f90:4469
    for (size_t s = 0; s < ns; ++s) {
        LeafPos P;
        if (c->tree.refined()) P = leaf_position(c->tree, K.leaf_node[(size_t)src_cell[s]]);
        else { std::memset(&P, 0, sizeof P); P.base = (int32_t)src_cell[s]; }
        expansion_star_centre(P, c->n, &star[s].x, &star[s].y, &star[s].z);
        star[s].r2 = expansion_cull_r2(params[3 * s], c->box);
        test[s].radius = params[3 * s];
        test[s].coef = params[3 * s + 1];
        test[s].limit = margin * params[3 * s + 2];
        test[s].reserved_ = 0.0;
    }

    FTTE_HIP(c, K.exp_star.reserve(ns));
    FTTE_HIP(c, K.exp_test.reserve(ns));
    FTTE_HIP(c, K.counters.reserve(4));
    if (rho_coef) FTTE_HIP(c, K.out.reserve(nc));
    const unsigned long long zero[4] = {0ull, 0ull, 0ull, 0ull};
    FTTE_HIP(c, hipMemcpyAsync(K.exp_star, star.data(), sizeof(ExpStar) * ns, hipMemcpyHostToDevice, c->stream));
    FTTE_HIP(c, hipMemcpyAsync(K.exp_test, test.data(), sizeof(ExpStarTest) * ns, hipMemcpyHostToDevice, c->stream));
    FTTE_HIP(c, hipMemcpyAsync(K.counters, zero, sizeof zero, hipMemcpyHostToDevice, c->stream));
    ExpandRec R;
    std::memset(&R, 0, sizeof R);
    R.star = K.exp_star; R.test = K.exp_test;
    R.pos = c->tree.refined() ? K.leaf_pos.get() : nullptr;
    R.rho = G.field(GasState::kRho); R.HI = G.field(GasState::kHI); R.HeI = G.field(GasState::kHeI); R.HeII = G.field(GasState::kHeII);
    R.rho_coef = rho_coef ? K.out.get() : nullptr;
    R.counters = K.counters;
    R.ncell = c->ncell; R.n = c->n; R.nsrc = nsrc; R.box = c->box;
    for (int l = 0; l < kExpMaxLevels; ++l) R.shift[l] = expansion_shift(l, c->n);
    // from here on the medium changes: whatever happens, the tracer's packed copy is stale
    G.species_changed();
    if (launch_expansion(R, c->stream.get())) return fail(c, FTTE_ERR_NO_DEVICE, who + "kernel launch failed");
    unsigned long long out[4];
    FTTE_HIP(c, hipMemcpyAsync(out, K.counters, sizeof out, hipMemcpyDeviceToHost, c->stream));
    if (rho_coef) FTTE_HIP(c, hipMemcpyAsync(rho_coef, K.out, sizeof(double) * nc, hipMemcpyDeviceToHost, c->stream));
    FTTE_HIP(c, hipStreamSynchronize(c->stream));
    K.expansion_tests = (long long)out[0];
    if (nchanged) *nchanged = (int64_t)out[1];
    return FTTE_OK;
}

int ftte_get_density(ftte_ctx *c, double *rho)
{
    int rc = check_ready(c, false);
    if (rc) return rc;
    if (!rho) return fail(c, FTTE_ERR_ARG, "ftte_get_density: bad argument");
    if (!c->gas.ready_with_density(c->ncell)) return fail(c, FTTE_ERR_STATE, "ftte_get_density: no medium with density (ftte_set_medium with rho)");
    FTTE_HIP(c, hipSetDevice(c->device));
    FTTE_HIP(c, hipMemcpyAsync(rho, c->gas.field(GasState::kRho), sizeof(double) * (size_t)c->ncell, hipMemcpyDeviceToHost, c->stream));
    FTTE_HIP(c, hipStreamSynchronize(c->stream));
    return FTTE_OK;
}

int ftte_compute_opacities(ftte_ctx *c, int nnu, const double *beta)
{
    int rc = check_ready(c, false);
    if (rc) return rc;
    if (nnu < 1 || !beta) return fail(c, FTTE_ERR_ARG, "ftte_compute_opacities: bad argument");
    const GasState &G = c->gas;
    if (!G.ready(c->ncell)) return fail(c, FTTE_ERR_STATE, "no medium: call ftte_set_medium first");
    FTTE_HIP(c, hipSetDevice(c->device));
    if ((rc = wait_sweep(c))) return rc;
    FTTE_HIP(c, hipStreamSynchronize(c->stream));
    if ((rc = ensure_kappa(c, nnu))) return rc;
    DeviceBuffer<double> dbeta;
    FTTE_HIP(c, dbeta.reserve(3 * (size_t)nnu));
    hipError_t e = hipMemcpyAsync(dbeta, beta, sizeof(double) * 3 * nnu, hipMemcpyHostToDevice, c->stream);
    int lrc = 0;
    if (e == hipSuccess)
        lrc = launch_opacity(G.field(GasState::kHI), G.field(GasState::kHeI), G.field(GasState::kHeII), dbeta, c->kappa.source(), (long)c->ncell, nnu, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e != hipSuccess) return fail(c, FTTE_ERR_NO_DEVICE, std::string("ftte_compute_opacities: ") + hipGetErrorString(e));
    if (lrc) return fail(c, FTTE_ERR_NO_DEVICE, "ftte_compute_opacities: kernel launch failed");
    c->nnu = nnu;
    c->kappa.set();
    return FTTE_OK;
}

int ftte_assign_uvb_radiation(ftte_ctx *c, int nnu, const double *uvb, double self_shielding_threshold, double *J)
{
    return assign_uvb(c, nnu, uvb, self_shielding_threshold, J, false, "ftte_assign_uvb_radiation");
}

int ftte_assign_uvb_radiation_device(ftte_ctx *c, int nnu, const double *uvb, double self_shielding_threshold, double *J_dev)
{
    return assign_uvb(c, nnu, uvb, self_shielding_threshold, J_dev, true, "ftte_assign_uvb_radiation_device");
}

} // extern "C"
