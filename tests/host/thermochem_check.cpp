// thermochem_check.cpp -- the coupled step of radiativetransfer_amd/csrc/ftte_thermochem_math.h evaluated on the host.  One source,
// two builds (tests/test_thermochem_host.py, tests/_thermochem.py):
//   * a shared library without sanitizers: tc_advance loops thermochem_advance_cell over arrays handed in through ctypes -- what the
//     Python tests and the bitwise GPU tests compare against -- and tc_pair is the existing pair, chem_advance_cell(h, 1) at a GIVEN
//     logarithm and then thermal_advance_cell(h, 1) on the new species, which is what a subcycle must equal;
//   * a program: main() drives the step over a field of random cells in every rate mode and checks, in every leaf, the fraction
//     bounds, the cap, and -- for the uniform schedule, where the last subcycle can be made again from outside -- the root property of
//     the last temperature step; built with -fsanitize=address,undefined.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <limits>
#include <vector>

#include "fit_tables.h"
#include "ftte_thermochem_math.h"

namespace {
const ftte_consts kMath = FTTE_CONSTS_INIT;
}

extern "C" {

// thermochem_advance_cell over ncell cells.  logtem: the stored logarithm per cell.  rates: [6][ncell] krate24..26, crate24..26 per
// cell, or NULL; J: [3][ncell] when run_uvb; k: [6][nratec]; cool: [13][nratec]; hydro: the stored hydroHeating to add, or NULL.
// Every output is written for every cell.  Returns 1 + the first failing cell, or 0.
long long tc_advance(long long ncell, int n, const int32_t *level, double box, const double *rho, const double *tgas, const double *logtem,
                     const double *HI, const double *HeI, const double *HeII, const double *rates, int run_uvb, const double *J, const double *ksi,
                     const double *gamma, const double *uniform, const double *uniform_gamma, double threshold, int nratec, double logtem0,
                     double logtem9, double dlogtem, const double *k, const double *cool, double comp1, double comp2, const double *hydro, double dt,
                     double eta, int max_subcycles, double tmin, double tmax, double *HI_out, double *HeI_out, double *HeII_out, double *T_out,
                     double *logtem_out, long long *steps, int32_t *subcycles, int32_t *capped, double *change, double *tchange)
{
    const ChemTable T = {k, nratec, logtem0, logtem9, dlogtem};
    const ThermalTable C = {cool, nratec, 1};
    long long first_bad = 0;
    for (long long c = 0; c < ncell; ++c) {
        unsigned long long s;
        int sub, cap;
        double r[6] = {0., 0., 0., 0., 0., 0.};
        if (rates) for (int i = 0; i < 6; ++i) r[i] = rates[i * ncell + c];
        const int ok = thermochem_advance_cell(&kMath, &T, &C, rho[c], tgas[c], logtem[c], HI[c], HeI[c], HeII[c], chem_cell_volume(box, level[c], n),
                                               rates != nullptr, r[0], r[1], r[2], r[3], r[4], r[5], run_uvb ? J + c : nullptr, (long)ncell, ksi, uniform,
                                               gamma, uniform_gamma, threshold, comp1, comp2, hydro ? hydro[c] : 0., dt, eta, max_subcycles, tmin, tmax,
                                               &HI_out[c], &HeI_out[c], &HeII_out[c], &T_out[c], &logtem_out[c], &s, &sub, &cap, &change[c], &tchange[c]);
        steps[c] = (long long)s;
        subcycles[c] = sub;
        capped[c] = cap;
        if (!ok && !first_bad) first_bad = c + 1;
    }
    return first_bad;
}

// The existing pair over h at a given logarithm: chem_advance_cell(h, 1), then thermal_advance_cell(h, 1) from tgas on the new
// species.  Out: the species, the temperature and its ftte_log.  Returns 1 + the first failing cell, or 0.
long long tc_pair(long long ncell, int n, const int32_t *level, double box, const double *rho, const double *tgas, const double *logtem,
                  const double *HI, const double *HeI, const double *HeII, const double *rates, int run_uvb, const double *J, const double *ksi,
                  const double *gamma, const double *uniform, const double *uniform_gamma, double threshold, int nratec, double logtem0,
                  double logtem9, double dlogtem, const double *k, const double *cool, double comp1, double comp2, double h, double tmin, double tmax,
                  double *HI_out, double *HeI_out, double *HeII_out, double *T_out, double *logtem_out)
{
    const ChemTable T = {k, nratec, logtem0, logtem9, dlogtem};
    const ThermalTable C = {cool, nratec, 1};
    long long first_bad = 0;
    for (long long c = 0; c < ncell; ++c) {
        unsigned long long s;
        double change, r[6] = {0., 0., 0., 0., 0., 0.};
        if (rates) for (int i = 0; i < 6; ++i) r[i] = rates[i * ncell + c];
        const double vol = chem_cell_volume(box, level[c], n);
        const double *Jc = run_uvb ? J + c : nullptr;
        int ok = chem_advance_cell(&T, rho[c], logtem[c], HI[c], HeI[c], HeII[c], vol, rates != nullptr, r[0], r[1], r[2], Jc, (long)ncell, ksi, uniform,
                                   threshold, h, 1, &HI_out[c], &HeI_out[c], &HeII_out[c], &s, &change);
        ok = thermal_advance_cell(&kMath, &T, &C, rho[c], tgas[c], HI_out[c], HeI_out[c], HeII_out[c], vol, rates != nullptr, r[3], r[4], r[5], Jc,
                                  (long)ncell, gamma, uniform_gamma, threshold, comp1, comp2, 0., h, 1, tmin, tmax, &T_out[c], &logtem_out[c], &s,
                                  &change) && ok;
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

} // namespace

int main()
{
    const int nratec = 400, n = 8;
    const long long nc = (long long)n * n * n; // 512 cells
    const double logtem0 = std::log(1.), logtem9 = std::log(1e8), dlogtem = (logtem9 - logtem0) / (nratec - 1), box = 2.5e23;
    std::vector<double> k, cool;
    fill_tables(nratec, logtem0, dlogtem, k, cool);
    const ChemTable T = {k.data(), nratec, logtem0, logtem9, dlogtem};
    const ThermalTable C = {cool.data(), nratec, 1};
    Lcg rng{2025};
    std::vector<int32_t> level((size_t)nc, 0);
    std::vector<double> rho((size_t)nc), tgas((size_t)nc), lt0((size_t)nc), HI((size_t)nc), HeI((size_t)nc), HeII((size_t)nc), rates(6 * (size_t)nc),
        J(3 * (size_t)nc);
    const double vol = chem_cell_volume(box, 0, n);
    for (long long c = 0; c < nc; ++c) {
        rho[c] = std::pow(10., rng.between(-27.5, -22.5));
        tgas[c] = std::pow(10., rng.between(-0.5, 8.5)); // beyond both ends of the table
        lt0[c] = std::log(tgas[c]);
        const double nh = chem_nh(rho[c]), nhe = chem_nhe(rho[c]);
        HI[c] = nh * std::pow(10., rng.between(-8., 0.1));
        HeI[c] = nhe * rng.between(0., 1.2); // HeI + HeII > nhe in many cells, HeI > nhe in some
        HeII[c] = nhe * rng.between(0., 1.2);
        for (int r = 0; r < 3; ++r) {
            const bool lit = rng.next() < 0.3;
            rates[r * nc + c] = lit ? std::pow(10., rng.between(-16., -11.)) * vol * nh : 0.;
            rates[(3 + r) * nc + c] = lit ? std::pow(10., rng.between(-27., -22.)) * vol * nh : 0.;
            J[r * nc + c] = std::pow(10., rng.between(-24., -21.));
        }
    }
    const double ksi[9] = {2.0e9, 0., 0., 1.5e9, 0., 1.2e9, 4.0e8, 3.0e8, 5.0e8}, gamma[9] = {2.0e-2, 0., 0., 1.5e-2, 1.2e-2, 0., 4.0e-3, 5.0e-3, 3.0e-3};
    const double uniform[3] = {3e-14, 1e-16, 2e-14}, uniform_gamma[3] = {3e-25, 1e-27, 2e-25}, threshold = 3e21;
    const double comp1 = 5.65e-36 * 1e4, comp2 = FTTE_T_CMB * 10., tmin = 1., tmax = 1e9;
    std::vector<double> a((size_t)nc), b((size_t)nc), d((size_t)nc), T1((size_t)nc), lt((size_t)nc), change((size_t)nc), tchange((size_t)nc);
    std::vector<long long> steps((size_t)nc);
    std::vector<int32_t> sub((size_t)nc), cap((size_t)nc);

    // every rate mode, short and long steps, adaptive, uniform and capped schedules: the bounds and the cap in every leaf
    struct Run { double dt, eta; int max_sub; };
    const Run runs[] = {{1e9, 0.1, 64}, {1e13, 0.1, 64}, {1e13, 0., 3}, {1e40, 0.5, 8}, {1e13, 1e-6, 8}};
    long long ones = 0, full = 0;
    for (int mode = 0; mode < 3; ++mode) // J, J + point rates, uniform background + point rates
        for (const Run &R : runs) {
            const double *pr = mode ? rates.data() : nullptr;
            const long long bad = tc_advance(nc, n, level.data(), box, rho.data(), tgas.data(), lt0.data(), HI.data(), HeI.data(), HeII.data(), pr,
                                             mode < 2, J.data(), ksi, gamma, uniform, uniform_gamma, threshold, nratec, logtem0, logtem9, dlogtem,
                                             k.data(), cool.data(), comp1, comp2, nullptr, R.dt, R.eta, R.max_sub, tmin, tmax, a.data(), b.data(),
                                             d.data(), T1.data(), lt.data(), steps.data(), sub.data(), cap.data(), change.data(), tchange.data());
            expect(bad == 0, "every cell gets through", bad - 1, R.dt, R.eta);
            for (long long c = 0; c < nc; ++c) {
                const double nh = chem_nh(rho[c]), nhe = chem_nhe(rho[c]);
                expect(a[c] >= -CHEM_ADVANCE_SLACK * nh && a[c] <= nh * (1. + CHEM_ADVANCE_SLACK), "HI within its budget", c, a[c], nh);
                expect(b[c] >= -CHEM_ADVANCE_SLACK * nhe && d[c] >= -CHEM_ADVANCE_SLACK * nhe && b[c] + d[c] <= nhe * (1. + CHEM_ADVANCE_SLACK),
                       "helium within its budget", c, b[c] + d[c], nhe);
                expect(T1[c] >= tmin && T1[c] <= tmax, "T within the clip", c, T1[c], tmax);
                expect(sub[c] >= 1 && sub[c] <= R.max_sub, "subcycles within the cap", c, (double)sub[c], (double)R.max_sub);
                // (with a step of its own a leaf may take max_sub subcycles unbounded, the last being what remained; not so at eta = 1e-6)
                expect(R.eta > 1e-6 || sub[c] < R.max_sub || cap[c], "a leaf that took them all was bounded by the cap", c, (double)sub[c], 0.);
                expect(R.eta > 0. || (sub[c] == R.max_sub && cap[c]), "the uniform schedule takes them all", c, (double)sub[c], 0.);
                ones += sub[c] == 1;
                full += sub[c] == R.max_sub;
            }
        }
    std::printf("cells x calls: %lld of one subcycle, %lld at the cap\n", ones, full);
    expect(ones > 0 && full > 0, "both ends occur", 0, (double)ones, (double)full);

    // the uniform schedule as a chain of pairs (J, no point rates): the same bits, and the root property of the last temperature step
    for (int N : {1, 3, 16}) {
        const double dt = 1e13;
        const long long bad = tc_advance(nc, n, level.data(), box, rho.data(), tgas.data(), lt0.data(), HI.data(), HeI.data(), HeII.data(), nullptr, 1,
                                         J.data(), ksi, gamma, uniform, uniform_gamma, 0., nratec, logtem0, logtem9, dlogtem, k.data(), cool.data(),
                                         comp1, comp2, nullptr, dt, 0., N, tmin, tmax, a.data(), b.data(), d.data(), T1.data(), lt.data(), steps.data(),
                                         sub.data(), cap.data(), change.data(), tchange.data());
        expect(bad == 0, "every cell gets through the uniform schedule", bad - 1, dt, N);
        std::vector<double> pa = HI, pb = HeI, pd = HeII, pT = tgas, pl = lt0, qa((size_t)nc), qb((size_t)nc), qd((size_t)nc), qT((size_t)nc), ql((size_t)nc);
        double remaining = dt, h = 0.;
        for (int s = 0; s < N; ++s) {
            h = std::fmin(remaining, std::fmax(0., remaining / (double)(N - s)));
            if (s) { qa = pa; qb = pb; qd = pd; qT = pT; ql = pl; }
            tc_pair(nc, n, level.data(), box, rho.data(), pT.data(), pl.data(), pa.data(), pb.data(), pd.data(), nullptr, 1, J.data(), ksi, gamma, uniform,
                    uniform_gamma, 0., nratec, logtem0, logtem9, dlogtem, k.data(), cool.data(), comp1, comp2, h, tmin, tmax, qa.data(), qb.data(),
                    qd.data(), qT.data(), ql.data());
            if (s + 1 < N) { pa = qa; pb = qb; pd = qd; pT = qT; pl = ql; }
            remaining = h >= remaining ? 0. : remaining - h;
        }
        expect(remaining == 0., "the schedule uses up dt exactly", 0, remaining, 0.);
        for (long long c = 0; c < nc; ++c) {
            expect(qa[c] == a[c] && qb[c] == b[c] && qd[c] == d[c], "species equal the chain of pairs", c, qa[c], a[c]);
            expect(qT[c] == T1[c] && ql[c] == lt[c], "temperature equals the chain of pairs", c, qT[c], T1[c]);
            // the last temperature step again: from pT on the final species over h
            ThermalCell q;
            const double Tin = N == 1 ? tgas[c] : pT[c];
            const int ok = thermal_advance_setup(&q, rho[c], Tin, a[c], b[c], d[c], vol, 0, 0., 0., 0., &J[c], (long)nc, gamma, uniform_gamma, 0., comp1,
                                                 comp2, 0., h, 1);
            expect(ok, "set-up", c, Tin, 0.);
            q.T0 = std::fmin(std::fmax(Tin, tmin), tmax);
            const double t1 = T1[c], F1 = thermal_F(&kMath, &T, &C, &q, t1);
            if (t1 == q.T0 && F1 == 0.) continue;
            if (t1 == tmax && F1 <= 0.) continue;
            if (t1 == tmin && F1 > 0.) continue;
            const double F2 = thermal_F(&kMath, &T, &C, &q, std::nextafter(t1, std::numeric_limits<double>::infinity()));
            expect(F1 <= 0. && F2 > 0., "the root property F(T1) <= 0 < F(next) of the last step", c, F1, F2);
        }
    }

    // a NaN temperature, a NaN density, an empty cell: named, and nothing else
    {
        std::vector<double> t2 = tgas, r2 = rho, r3 = rho;
        t2[37] = std::nan(""); r2[41] = std::nan(""); r3[43] = 0.;
        const double *tt[3] = {t2.data(), tgas.data(), tgas.data()}, *rr[3] = {rho.data(), r2.data(), r3.data()};
        const long long want[3] = {38, 42, 44};
        for (int i = 0; i < 3; ++i) {
            const long long bad = tc_advance(nc, n, level.data(), box, rr[i], tt[i], lt0.data(), HI.data(), HeI.data(), HeII.data(), rates.data(), i != 1,
                                             J.data(), ksi, gamma, uniform, uniform_gamma, threshold, nratec, logtem0, logtem9, dlogtem, k.data(),
                                             cool.data(), comp1, comp2, nullptr, 1e13, 0.1, 16, tmin, tmax, a.data(), b.data(), d.data(), T1.data(),
                                             lt.data(), steps.data(), sub.data(), cap.data(), change.data(), tchange.data());
            expect(bad == want[i], "the bad cell is named", bad - 1, (double)want[i] - 1., 0.);
            for (long long c = 0; c < nc; ++c) expect(sub[c] >= 0 && sub[c] <= 16, "subcycles within the cap, bad cell included", c, (double)sub[c], 16.);
        }
    }

    if (failures) { std::printf("coupled step under the sanitizers: %d FAILED\n", failures); return 1; }
    std::printf("coupled step under the sanitizers: ok\n");
    return 0;
}
