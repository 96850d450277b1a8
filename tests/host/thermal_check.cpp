// thermal_check.cpp -- the thermal balance of radiativetransfer_amd/csrc/ftte_thermal_math.h evaluated on the host.  One source, two
// builds (tests/test_thermal_host.py, tests/_thermal.py):
//   * a program: main() drives the temperature step over a field of random cells -- densities over five decades, temperatures over
//     the table's whole span and beyond both ends, species mixes that overfill the helium budget, mean intensities over three
//     decades, point-source heating in some cells, steps of 1e9, 1e13 and 1e40 s in 1 and 3 substeps -- and checks the root
//     property of the step or its documented clamp in every cell; built with -fsanitize=address,undefined;
//   * a shared library without sanitizers: th_log, th_equilibrium and th_advance loop the header over arrays handed in through
//     ctypes, which is what the Python tests and the bitwise GPU tests compare against.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <limits>
#include <vector>

#include "ftte_thermal_math.h"

namespace {
const ftte_consts kMath = FTTE_CONSTS_INIT;
}

extern "C" {

void th_log(long long count, const double *x, double *out)
{
    for (long long i = 0; i < count; ++i) out[i] = ftte_log(&kMath, x[i]);
}

// thermal_equilibrium_cell over ncell cells, at logtem[c] or (logtem NULL) at ftte_log(tgas[c]).  crate: [3][ncell] crate24, crate25,
// crate26 per cell, or NULL; J: [3][ncell] when run_uvb; cool: [13][nratec].  Returns 1 + the first failing cell (temperature not
// positive and finite, or a result not finite), or 0.
long long th_equilibrium(long long ncell, int n, const int32_t *level, double box, const double *rho, const double *tgas, const double *logtem,
                         const double *HI, const double *HeI, const double *HeII, const double *crate, int run_uvb, const double *J,
                         const double *gamma, const double *uniform, double threshold, int nratec, double logtem0, double logtem9, double dlogtem,
                         const double *cool, double comp1, double comp2, double *heating, double *cooling, double *hydro)
{
    const ChemTable T = {nullptr, nratec, logtem0, logtem9, dlogtem};
    const ThermalTable C = {cool, nratec, 1};
    long long first_bad = 0;
    for (long long c = 0; c < ncell; ++c) {
        int ok = tgas[c] > 0. && thermal_finite(tgas[c]);
        heating[c] = cooling[c] = hydro[c] = 0.;
        if (ok) {
            hydro[c] = thermal_equilibrium_cell(&T, &C, rho[c], tgas[c], logtem ? logtem[c] : ftte_log(&kMath, tgas[c]), HI[c], HeI[c], HeII[c],
                                                chem_cell_volume(box, level[c], n), crate != nullptr, crate ? crate[c] : 0.,
                                                crate ? crate[ncell + c] : 0., crate ? crate[2 * ncell + c] : 0., run_uvb ? J + c : nullptr,
                                                (long)ncell, gamma, uniform, threshold, comp1, comp2, &heating[c], &cooling[c]);
            ok = thermal_finite(heating[c]) && thermal_finite(cooling[c]) && thermal_finite(hydro[c]);
        }
        if (!ok && !first_bad) first_bad = c + 1;
    }
    return first_bad;
}

// thermal_advance_cell over ncell cells; hydro: the stored hydroHeating per cell to add, or NULL.  Out (written for every cell,
// failing ones included): the temperature, its ftte_log, steps[ncell], change[ncell].  Returns 1 + the first failing cell, or 0.
long long th_advance(long long ncell, int n, const int32_t *level, double box, const double *rho, const double *tgas, const double *HI,
                     const double *HeI, const double *HeII, const double *crate, int run_uvb, const double *J, const double *gamma,
                     const double *uniform, double threshold, int nratec, double logtem0, double logtem9, double dlogtem, const double *cool,
                     double comp1, double comp2, const double *hydro, double dt, int substeps, double tmin, double tmax, double *T_out,
                     double *logtem_out, long long *steps, double *change)
{
    const ChemTable T = {nullptr, nratec, logtem0, logtem9, dlogtem};
    const ThermalTable C = {cool, nratec, 1};
    long long first_bad = 0;
    for (long long c = 0; c < ncell; ++c) {
        unsigned long long s;
        const int ok = thermal_advance_cell(&kMath, &T, &C, rho[c], tgas[c], HI[c], HeI[c], HeII[c], chem_cell_volume(box, level[c], n),
                                            crate != nullptr, crate ? crate[c] : 0., crate ? crate[ncell + c] : 0.,
                                            crate ? crate[2 * ncell + c] : 0., run_uvb ? J + c : nullptr, (long)ncell, gamma, uniform, threshold,
                                            comp1, comp2, hydro ? hydro[c] : 0., dt, substeps, tmin, tmax, &T_out[c], &logtem_out[c], &s,
                                            &change[c]);
        steps[c] = (long long)s;
        if (!ok && !first_bad) first_bad = c + 1;
    }
    return first_bad;
}

// chem_solve_cell (the equilibrium update) over ncell cells at a GIVEN logtem -- what the chemistry reads after a temperature step --
// with the transfer's J and no point rates.  Returns 1 + the first cell the reference would stop at, or 0.
long long th_solve(long long ncell, int n, const int32_t *level, double box, const double *rho, const double *logtem, const double *HI,
                   const double *HeI, const double *HeII, const double *J, const double *ksi, int nratec, double logtem0, double logtem9,
                   double dlogtem, const double *k, double *HI_out, double *HeI_out, double *HeII_out)
{
    const ChemTable T = {k, nratec, logtem0, logtem9, dlogtem};
    long long first_bad = 0;
    for (long long c = 0; c < ncell; ++c) {
        unsigned steps;
        int tame;
        double change;
        const int ok = chem_solve_cell(&T, rho[c], logtem[c], HI[c], HeI[c], HeII[c], chem_cell_volume(box, level[c], n), 0, 0., 0., 0., J + c,
                                       (long)ncell, ksi, nullptr, 0., &HI_out[c], &HeI_out[c], &HeII_out[c], &steps, &change, &tame);
        if (!ok && !first_bad) first_bad = c + 1;
    }
    return first_bad;
}

} // extern "C"

namespace {

int failures = 0;

void expect(bool ok, const char *what, long long cell, double a, double b)
{
    if (ok) return;
    if (++failures <= 20) std::printf("FAILED %s: cell %lld, %.17g vs %.17g\n", what, cell, a, b);
}

// cooling coefficients of the usual shape (fits in the public literature: Black 1981, MNRAS 197, 553; Cen 1992, ApJS 78, 341), only
// to have a table whose rows span what a real one spans -- exponential cut-offs at low temperature, recombination falling with
// temperature, a cooling curve that is not monotonic
void fill_table(int nratec, double logtem0, double dlogtem, std::vector<double> &c)
{
    c.assign(13 * (size_t)nratec, 0.);
    for (int i = 0; i < nratec; ++i) {
        const double T = std::exp(logtem0 + i * dlogtem), s = std::sqrt(T), f = 1. / (1. + std::sqrt(T / 1e5));
        const double row[13] = {7.5e-19 * std::exp(-118348. / T) * f,
                                9.1e-27 * std::exp(-13179. / T) * std::pow(T, -0.1687) * f,
                                5.54e-17 * std::exp(-473638. / T) * std::pow(T, -0.397) * f,
                                1.27e-21 * s * std::exp(-157809.1 / T) * f,
                                9.38e-22 * s * std::exp(-285335.4 / T) * f,
                                5.01e-27 * std::pow(T, -0.1687) * f * std::exp(-55338. / T),
                                4.95e-22 * s * std::exp(-631515. / T) * f,
                                8.70e-27 * s * std::pow(T / 1e3, -0.2) / (1. + std::pow(T / 1e6, 0.7)),
                                1.55e-26 * std::pow(T, 0.3647),
                                1.24e-13 * std::pow(T, -1.5) * std::exp(-470000. / T) * (1. + 0.3 * std::exp(-94000. / T)),
                                3.48e-26 * s * std::pow(T / 1e3, -0.2) / (1. + std::pow(T / 1e6, 0.7)),
                                1.43e-27 * s * (1.1 + 0.34 * std::exp(-(5.5 - std::log10(T)) * (5.5 - std::log10(T)) / 3.)),
                                7.5e-19 * std::exp(-118348. / T) * f};
        for (int r = 0; r < 13; ++r) c[(size_t)r * nratec + i] = row[r];
    }
}

struct Lcg { // (no <random>: the same field everywhere)
    uint64_t s;
    double next() { s = s * 6364136223846793005ull + 1442695040888963407ull; return (double)(s >> 11) * 0x1p-53; }
    double between(double a, double b) { return a + (b - a) * next(); }
};

} // namespace

int main()
{
    const int nratec = 400, n = 16;
    const long long nc = (long long)n * n * n; // 4096 cells
    const double logtem0 = std::log(1.), logtem9 = std::log(1e8), dlogtem = (logtem9 - logtem0) / (nratec - 1), box = 2.5e23;
    std::vector<double> cool;
    fill_table(nratec, logtem0, dlogtem, cool);
    const ChemTable T = {nullptr, nratec, logtem0, logtem9, dlogtem};
    const ThermalTable C = {cool.data(), nratec, 1};
    Lcg rng{2024};
    std::vector<int32_t> level((size_t)nc, 0);
    std::vector<double> rho((size_t)nc), tgas((size_t)nc), HI((size_t)nc), HeI((size_t)nc), HeII((size_t)nc), crate(3 * (size_t)nc), J(3 * (size_t)nc);
    const double vol = chem_cell_volume(box, 0, n);
    for (long long c = 0; c < nc; ++c) {
        rho[c] = std::pow(10., rng.between(-27.5, -22.5));
        tgas[c] = std::pow(10., rng.between(-0.5, 8.5)); // beyond both ends of the table
        const double nh = chem_nh(rho[c]), nhe = chem_nhe(rho[c]);
        HI[c] = nh * std::pow(10., rng.between(-8., 0.1));
        HeI[c] = nhe * rng.between(0., 1.2); // HeI + HeII > nhe in many cells, HeI > nhe in some
        HeII[c] = nhe * rng.between(0., 1.2);
        for (int r = 0; r < 3; ++r) {
            crate[r * nc + c] = rng.next() < 0.3 ? std::pow(10., rng.between(-27., -22.)) * vol * nh : 0.;
            J[r * nc + c] = std::pow(10., rng.between(-24., -21.));
        }
    }
    // heating integrals of the size uvbBetaTable and uniformTable give [erg cm^2], a redshift-9 Compton term
    const double gamma[9] = {2.0e-2, 0., 0., 1.5e-2, 1.2e-2, 0., 4.0e-3, 5.0e-3, 3.0e-3}, uniform[3] = {3e-25, 1e-27, 2e-25}, threshold = 3e21;
    const double comp1 = 5.65e-36 * 1e4, comp2 = FTTE_T_CMB * 10., tmin = 1., tmax = 1e9;
    std::vector<double> T1((size_t)nc), lt((size_t)nc), change((size_t)nc), Ta((size_t)nc), Tb((size_t)nc);
    std::vector<long long> steps((size_t)nc), steps1((size_t)nc);

    long long clamped = 0, stationary = 0, bisected = 0;
    const double dts[] = {1e9, 1e13, 1e40};
    const int subs[] = {1, 3};
    for (int mode = 0; mode < 3; ++mode) // J, J + point heating, uniform background + point heating
        for (double dt : dts)
            for (int sub : subs) {
                const double *cr = mode ? crate.data() : nullptr;
                const int run_uvb = mode < 2;
                const long long bad = th_advance(nc, n, level.data(), box, rho.data(), tgas.data(), HI.data(), HeI.data(), HeII.data(), cr, run_uvb,
                                                 J.data(), gamma, uniform, threshold, nratec, logtem0, logtem9, dlogtem, cool.data(), comp1, comp2,
                                                 nullptr, dt, sub, tmin, tmax, T1.data(), lt.data(), steps.data(), change.data());
                expect(bad == 0, "every cell gets through", bad - 1, dt, sub);
                // the same call as `sub` calls of one substep each: the same temperatures, and each substep's own T0 to check against
                Ta = tgas;
                std::fill(steps1.begin(), steps1.end(), 0);
                for (int s = 0; s < sub; ++s) {
                    std::vector<long long> st((size_t)nc);
                    th_advance(nc, n, level.data(), box, rho.data(), Ta.data(), HI.data(), HeI.data(), HeII.data(), cr, run_uvb, J.data(), gamma, uniform,
                               threshold, nratec, logtem0, logtem9, dlogtem, cool.data(), comp1, comp2, nullptr, dt / sub, 1, tmin, tmax, Tb.data(),
                               lt.data(), st.data(), change.data());
                    for (long long c = 0; c < nc; ++c) {
                        steps1[c] += st[c];
                        ThermalCell q;
                        const int ok = thermal_advance_setup(&q, rho[c], Ta[c], HI[c], HeI[c], HeII[c], vol, cr != nullptr, cr ? cr[c] : 0.,
                                                             cr ? cr[nc + c] : 0., cr ? cr[2 * nc + c] : 0., run_uvb ? &J[c] : nullptr, (long)nc, gamma,
                                                             uniform, threshold, comp1, comp2, 0., dt / sub, 1);
                        expect(ok, "set-up", c, Ta[c], 0.);
                        q.T0 = std::fmin(std::fmax(Ta[c], tmin), tmax);
                        const double t1 = Tb[c], F1 = thermal_F(&kMath, &T, &C, &q, t1);
                        expect(t1 >= tmin && t1 <= tmax, "within the clip", c, t1, tmax);
                        expect(st[c] < CHEM_MAX_STEPS, "steps below the cap", c, (double)st[c], 0.);
                        if (t1 == q.T0 && F1 == 0.) { ++stationary; continue; }                 // rule 1
                        if (t1 == tmax && F1 <= 0.) { ++clamped; continue; }                   // rule 2's clamp
                        if (t1 == tmin && F1 > 0.) { ++clamped; continue; }                    // rule 3's clamp
                        const double up = std::nextafter(t1, std::numeric_limits<double>::infinity());
                        const double F2 = thermal_F(&kMath, &T, &C, &q, up);
                        expect(F1 <= 0. && F2 > 0., "the root property F(T1) <= 0 < F(next)", c, F1, F2);
                        // the root lies on the gas's own side of T0
                        const double F0 = thermal_F(&kMath, &T, &C, &q, q.T0);
                        expect(F0 < 0. ? t1 >= q.T0 : t1 <= q.T0, "the root is on the gas's own side of T0", c, t1, q.T0);
                        ++bisected;
                    }
                    Ta = Tb;
                }
                for (long long c = 0; c < nc; ++c) {
                    expect(Ta[c] == T1[c], "substeps equal a chain of calls", c, Ta[c], T1[c]);
                    expect(steps1[c] == steps[c], "steps of the substeps add up", c, (double)steps1[c], (double)steps[c]);
                }
            }
    std::printf("cells x calls: %lld bisected, %lld clamped, %lld stationary\n", bisected, clamped, stationary);
    expect(bisected > 10 * (clamped + stationary), "most cells bisect", 0, (double)bisected, (double)clamped);

    // a NaN temperature, a NaN density: reported as the failed cell, nothing else
    {
        std::vector<double> t2 = tgas, r2 = rho;
        t2[37] = std::nan("");
        long long bad = th_advance(nc, n, level.data(), box, rho.data(), t2.data(), HI.data(), HeI.data(), HeII.data(), nullptr, 1, J.data(), gamma, uniform,
                                   threshold, nratec, logtem0, logtem9, dlogtem, cool.data(), comp1, comp2, nullptr, 1e13, 2, tmin, tmax, T1.data(),
                                   lt.data(), steps.data(), change.data());
        expect(bad == 38, "the NaN temperature is named", bad - 1, 37., 0.);
        r2[41] = std::nan("");
        bad = th_advance(nc, n, level.data(), box, r2.data(), tgas.data(), HI.data(), HeI.data(), HeII.data(), crate.data(), 0, J.data(), gamma, uniform,
                         threshold, nratec, logtem0, logtem9, dlogtem, cool.data(), comp1, comp2, nullptr, 1e13, 2, tmin, tmax, T1.data(), lt.data(),
                         steps.data(), change.data());
        expect(bad == 42, "the NaN density is named", bad - 1, 41., 0.);
        std::vector<double> h((size_t)nc), k((size_t)nc), y((size_t)nc);
        bad = th_equilibrium(nc, n, level.data(), box, r2.data(), t2.data(), nullptr, HI.data(), HeI.data(), HeII.data(), nullptr, 0, nullptr, gamma, uniform,
                             threshold, nratec, logtem0, logtem9, dlogtem, cool.data(), comp1, comp2, h.data(), k.data(), y.data());
        expect(bad == 38, "thermal equilibrium names the NaN temperature", bad - 1, 37., 0.);
    }

    if (failures) { std::printf("thermal step under the sanitizers: %d FAILED\n", failures); return 1; }
    std::printf("thermal step under the sanitizers: ok\n");
    return 0;
}
