// recombination_check.cpp -- the diffuse recombination source of radiativetransfer_amd/csrc/ftte_recombination_math.h evaluated on the
// host.  One source, two builds (tests/test_recombination_host.py, tests/_recombination.py):
//   * a program: main() runs the statement over a field of random cells -- densities over five decades, temperatures beyond both
//     ends of the table, species that overfill their budgets, fully ionised and fully neutral cells -- and checks in every cell
//     that S is finite and not negative, that 4 pi S D gives back E, and that the lost pairs are exactly those that emit where
//     nothing absorbs; a NaN and a zero density are named; built with -fsanitize=address,undefined;
//   * a shared library without sanitizers: rc_source loops the header over arrays handed in through ctypes, which is what the
//     Python tests and the bitwise GPU tests compare against.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "ftte_recombination_math.h"

extern "C" {

// recomb_source_cell over ncell cells.  g: [3][nratec]; ksi: [group][24, 25, 26]; share: [ion][group]; S, E: [3][ncell] (E may be
// NULL); *lost: the (cell, group) pairs lost, over the cells that got through.  Returns 1 + the first failing cell, or 0.
long long rc_source(long long ncell, const double *rho, const double *logtem, const double *HI, const double *HeI, const double *HeII, int nratec,
                    double logtem0, double logtem9, double dlogtem, const double *g, const double *ksi, const double *share, double *S, double *E,
                    long long *lost)
{
    const ChemTable T = {g, nratec, logtem0, logtem9, dlogtem};
    long long first_bad = 0, count = 0;
    for (long long c = 0; c < ncell; ++c) {
        double s[3], e[3];
        int n;
        const int ok = recomb_source_cell(&T, rho[c], logtem[c], HI[c], HeI[c], HeII[c], ksi, share, s, e, &n);
        for (int j = 0; j < 3; ++j) {
            S[j * ncell + c] = s[j];
            if (E) E[j * ncell + c] = e[j];
        }
        if (ok) count += n;
        else if (!first_bad) first_bad = c + 1;
    }
    *lost = count;
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

struct Lcg { // (no <random>: the same field everywhere)
    uint64_t s;
    double next() { s = s * 6364136223846793005ull + 1442695040888963407ull; return (double)(s >> 11) * 0x1p-53; }
    double between(double a, double b) { return a + (b - a) * next(); }
};

} // namespace

int main()
{
    const int nratec = 400;
    const long long nc = 4096;
    const double logtem0 = std::log(1.), logtem9 = std::log(1e8), dlogtem = (logtem9 - logtem0) / (nratec - 1);
    // coefficients of the usual shape: power laws falling with temperature, the helium row zero at the cold end as a difference of
    // two fits clipped at zero is
    std::vector<double> g(3 * (size_t)nratec);
    for (int i = 0; i < nratec; ++i) {
        const double T = std::exp(logtem0 + i * dlogtem);
        g[i] = 1.6e-13 * std::pow(T / 1e4, -0.55);
        g[nratec + i] = T < 300. ? 0. : 1.5e-13 * std::pow(T / 1e4, -0.6);
        g[2 * nratec + i] = 9.0e-13 * std::pow(T / 1e4, -0.6);
    }
    Lcg rng{4711};
    std::vector<double> rho((size_t)nc), lt((size_t)nc), HI((size_t)nc), HeI((size_t)nc), HeII((size_t)nc), S(3 * (size_t)nc), E(3 * (size_t)nc);
    for (long long c = 0; c < nc; ++c) {
        rho[c] = std::pow(10., rng.between(-27.5, -22.5));
        lt[c] = std::log(std::pow(10., rng.between(-0.5, 8.5))); // beyond both ends of the table
        const double nh = chem_nh(rho[c]), nhe = chem_nhe(rho[c]);
        HI[c] = nh * std::pow(10., rng.between(-8., 0.1));
        HeI[c] = nhe * rng.between(0., 1.2); // HeI + HeII > nhe in many cells, HeI > nhe in some
        HeII[c] = nhe * rng.between(0., 1.2);
        if (c % 16 == 3) HI[c] = 0.;                                  // nothing absorbs group 0
        if (c % 16 == 7) { HI[c] = nh; HeI[c] = nhe; HeII[c] = 0.; } // neutral
        if (c % 16 == 11) { HI[c] = 0.; HeI[c] = 0.; HeII[c] = 0.; } // fully ionised: every group lost
    }
    const double ksi[9] = {2.1e6, 0., 0., 6.0e5, 0., 1.7e6, 9.0e4, 3.0e5, 4.0e5};
    const double shares[2][9] = {{1., 0., 0., 0., 1., 0., 0., 0., 1.}, {0.7, 0.2, 0.1, 0., 0.6, 0.3, 0.1, 0.1, 0.8}};
    for (const double *share : {shares[0], shares[1]}) {
        long long lost = -1, want_lost = 0, emitting = 0;
        const long long bad = rc_source(nc, rho.data(), lt.data(), HI.data(), HeI.data(), HeII.data(), nratec, logtem0, logtem9, dlogtem, g.data(), ksi,
                                        share, S.data(), E.data(), &lost);
        expect(bad == 0, "every cell gets through", bad - 1, 0., 0.);
        for (long long c = 0; c < nc; ++c) {
            const double nh = chem_nh(rho[c]), nhe = chem_nhe(rho[c]);
            const double hi = std::fmax(std::fmin(HI[c], nh), 0.), hei = std::fmax(std::fmin(HeI[c], nhe), 0.),
                         heii = std::fmax(std::fmin(HeII[c], nhe - hei), 0.);
            const double D[3] = {hi * ksi[0], hi * ksi[3] + hei * ksi[5], hi * ksi[6] + heii * ksi[7] + hei * ksi[8]};
            for (int j = 0; j < 3; ++j) {
                const double s = S[j * nc + c], e = E[j * nc + c];
                expect(recomb_finite(s) && s >= 0. && e >= 0., "S and E finite and not negative", c, s, e);
                if (D[j] == 0.) { expect(s == 0., "S is 0 where nothing absorbs", c, s, 0.); want_lost += e > 0.; }
                else expect(std::fabs(4. * FTTE_PI * s * D[j] - e) <= 4. * 0x1p-52 * e, "4 pi S D gives back E", c, 4. * FTTE_PI * s * D[j], e);
                emitting += e > 0.;
            }
            if (c % 16 == 7) expect(E[c] == 0. && E[nc + c] == 0. && E[2 * nc + c] == 0., "neutral gas emits nothing", c, E[c], 0.);
        }
        expect(lost == want_lost && lost > nc / 16, "the lost pairs are those that emit where nothing absorbs", 0, (double)lost, (double)want_lost);
        expect(emitting > nc, "more pairs emit than there are cells (HeIII is clipped away in many)", 0, (double)emitting, (double)nc);
    }
    // a NaN density, a zero density: named, the first of them
    {
        std::vector<double> r2 = rho;
        long long lost;
        r2[41] = 0.;
        long long bad = rc_source(nc, r2.data(), lt.data(), HI.data(), HeI.data(), HeII.data(), nratec, logtem0, logtem9, dlogtem, g.data(), ksi, shares[0],
                                  S.data(), E.data(), &lost);
        expect(bad == 42, "the zero density is named", bad - 1, 41., 0.);
        r2[37] = std::nan("");
        bad = rc_source(nc, r2.data(), lt.data(), HI.data(), HeI.data(), HeII.data(), nratec, logtem0, logtem9, dlogtem, g.data(), ksi, shares[0], S.data(),
                        nullptr, &lost);
        expect(bad == 38, "the NaN density is named", bad - 1, 37., 0.);
    }
    if (failures) { std::printf("recombination source under the sanitizers: %d FAILED\n", failures); return 1; }
    std::printf("recombination source under the sanitizers: ok\n");
    return 0;
}
