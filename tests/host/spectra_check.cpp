// spectra_check.cpp -- the absorption line of radiativetransfer_amd/csrc/ftte_spectra_math.h evaluated on the host.  One source, two
// builds (tests/test_spectra_host.py, tests/_spectra.py):
//   * a shared library without sanitizers: sp_profile is H(a, x) over an array, sp_lines the header's loop over sightlines given as
//     segment lists (the leaves the numpy walk of tests/_spectra.py finds), which is what the Python tests and the bitwise GPU tests
//     compare against;
//   * with -DSPECTRA_CHECK_MAIN a program: main(argc, argv) reads segment lists from a file the test writes from the goldens (or
//     makes random ones without a file), runs sp_lines over them with windows that put cores inside, at the edge of and outside the
//     spectrum, with and without damping, period and Hubble flow, and checks that every tau is finite and not negative, that the
//     summaries are those of the finished tau, and that a leaf without a line width is named; built with
//     -fsanitize=address,undefined.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "ftte_spectra_math.h"

static const ftte_consts kMath = FTTE_CONSTS_INIT;

extern "C" {

// H(a, x) for n values of x
void sp_profile(long long n, const double *x, double a, double *H)
{
    for (long long q = 0; q < n; ++q) {
        const double x2 = x[q] * x[q];
        H[q] = spectra_voigt(a, x2, spectra_gauss(&kMath, x2));
    }
}

// the wing alone, and the whole form with H0 = 0, for n values of x^2 beyond the core
void sp_wing(long long n, const double *x2, double a, double *wing, double *whole)
{
    for (long long q = 0; q < n; ++q) {
        wing[q] = spectra_wing(a, x2[q]);
        whole[q] = spectra_voigt(a, x2[q], 0.0);
    }
}

// par[9] = {v0, dv, hubble, period, sigma_line, damping, mass, b_turb, unused}.  Sightline L has segments off[L] .. off[L+1]-1 in
// its order: density, size [cm], temperature, centre s [cm], line-of-sight velocity u.  tau: [nline][nvel] or NULL; summary:
// [nline][3] = N, W, dv90 or NULL.  Returns 1 + the first segment without a line width (nothing is written then), or 0.
long long sp_lines(long long nline, const long long *off, const double *dens, const double *size, const double *tgas, const double *s,
                   const double *u, const double *par, long long nvel, double *tau, double *summary)
{
    ftte_spectra_par P;
    P.v0 = par[0]; P.dv = par[1]; P.hubble = par[2];
    P.period = par[3]; P.inv_period = par[3] > 0.0 ? 1.0 / par[3] : 0.0;
    P.sigma = par[4]; P.damping = par[5]; P.mass = par[6]; P.bturb = par[7];
    for (long long q = 0; q < off[nline]; ++q)
        if (!spectra_b2_ok(spectra_b2(&P, tgas[q]))) return q + 1;
    std::vector<double> line((size_t)nvel);
    for (long long L = 0; L < nline; ++L) {
        for (long long p = 0; p < nvel; ++p) line[(size_t)p] = 0.0;
        double N = 0.0;
        for (long long q = off[L]; q < off[L + 1]; ++q) {
            ftte_spectra_seg S;
            N = N + spectra_segment(&P, dens[q], size[q], tgas[q], s[q], u[q], &S);
            for (long long p = 0; p < nvel; ++p) line[(size_t)p] = spectra_accumulate(&kMath, &P, &S, spectra_pixel_velocity(&P, p), line[(size_t)p]);
        }
        if (tau)
            for (long long p = 0; p < nvel; ++p) tau[L * nvel + p] = line[(size_t)p];
        if (summary) {
            summary[3 * L] = N;
            spectra_summarise(&kMath, line.data(), nvel, P.dv, &summary[3 * L + 1], &summary[3 * L + 2]);
        }
    }
    return 0;
}

// W and dv90 of a given tau[nvel]
void sp_summarise(long long nvel, const double *tau, double dv, double *out2)
{
    spectra_summarise(&kMath, tau, nvel, dv, &out2[0], &out2[1]);
}

} // extern "C"

#ifdef SPECTRA_CHECK_MAIN
namespace {

int failures = 0;

void expect(bool ok, const char *what, long long at, double a, double b)
{
    if (ok) return;
    if (++failures <= 20) std::printf("FAILED %s: at %lld, %.17g vs %.17g\n", what, at, a, b);
}

struct Lcg { // (no <random>: the same lists everywhere)
    uint64_t s;
    double next() { s = s * 6364136223846793005ull + 1442695040888963407ull; return (double)(s >> 11) * 0x1p-53; }
    double between(double a, double b) { return a + (b - a) * next(); }
};

struct Lists {
    std::vector<long long> off;
    std::vector<double> dens, size, tgas, s, u;
};

// the file of tests/test_spectra_host.py: int64 nline, int64 off[nline + 1], then dens, size, tgas, s, u as doubles
bool read_lists(const char *path, Lists *L)
{
    std::FILE *f = std::fopen(path, "rb");
    if (!f) return false;
    long long nline = 0;
    bool ok = std::fread(&nline, sizeof nline, 1, f) == 1 && nline >= 1 && nline < (1ll << 24);
    if (ok) {
        L->off.resize((size_t)nline + 1);
        ok = std::fread(L->off.data(), sizeof(long long), L->off.size(), f) == L->off.size() && L->off[0] == 0;
        for (size_t q = 1; ok && q < L->off.size(); ++q) ok = L->off[q] >= L->off[q - 1];
        ok = ok && L->off.back() < (1ll << 28);
    }
    if (ok) {
        const size_t n = (size_t)L->off.back();
        for (std::vector<double> *v : {&L->dens, &L->size, &L->tgas, &L->s, &L->u}) {
            v->resize(n);
            ok = ok && std::fread(v->data(), sizeof(double), n, f) == n;
        }
    }
    std::fclose(f);
    return ok;
}

void random_lists(Lists *L)
{
    Lcg r{20261021ull};
    L->off.push_back(0);
    for (int line = 0; line < 40; ++line) {
        const int nseg = 1 + (int)(r.next() * 30);
        double pos = 0.0;
        for (int q = 0; q < nseg; ++q) {
            const double size = 3.0e22 * std::ldexp(1.0, -(int)(r.next() * 4));
            L->dens.push_back(std::pow(10.0, r.between(-9.0, -2.0)));
            L->size.push_back(size);
            L->tgas.push_back(std::pow(10.0, r.between(2.0, 6.0)));
            L->s.push_back(pos + 0.5 * size);
            L->u.push_back(r.between(-3.0e7, 3.0e7));
            pos += size;
        }
        L->off.push_back((long long)L->dens.size());
    }
}

void run(const Lists &L, const double *par, long long nvel)
{
    const long long nline = (long long)L.off.size() - 1;
    std::vector<double> tau((size_t)(nline * nvel)), summary((size_t)nline * 3), again((size_t)(nline * nvel));
    long long rc = sp_lines(nline, L.off.data(), L.dens.data(), L.size.data(), L.tgas.data(), L.s.data(), L.u.data(), par, nvel, tau.data(), summary.data());
    expect(rc == 0, "every leaf has a line width", rc, 0, 0);
    rc = sp_lines(nline, L.off.data(), L.dens.data(), L.size.data(), L.tgas.data(), L.s.data(), L.u.data(), par, nvel, again.data(), nullptr);
    for (size_t q = 0; q < tau.size(); ++q) {
        expect(std::isfinite(tau[q]) && tau[q] >= 0.0, "tau finite and not negative", (long long)q, tau[q], 0);
        expect(tau[q] == again[q], "the same tau without the summaries", (long long)q, tau[q], again[q]);
    }
    for (long long l = 0; l < nline; ++l) {
        double N = 0.0, out[2];
        for (long long q = L.off[l]; q < L.off[l + 1]; ++q) N = N + L.dens[(size_t)q] * L.size[(size_t)q];
        sp_summarise(nvel, &tau[(size_t)(l * nvel)], par[1], out);
        expect(summary[3 * l] == N, "N", l, summary[3 * l], N);
        expect(summary[3 * l + 1] == out[0] && out[0] >= 0.0 && out[0] <= (double)nvel * par[1] * (1 + 1e-12), "W", l, summary[3 * l + 1], out[0]);
        expect(summary[3 * l + 2] == out[1] && out[1] >= 0.0 && out[1] <= (double)(nvel - 1) * par[1], "dv90", l, summary[3 * l + 2], out[1]);
    }
}

} // namespace

int main(int argc, char **argv)
{
    Lists L;
    if (argc > 1) {
        if (!read_lists(argv[1], &L)) { std::printf("cannot read %s\n", argv[1]); return 2; }
    } else random_lists(&L);
    double lo = 1e300, hi = -1e300;
    for (double u : L.u) { lo = u < lo ? u : lo; hi = u > hi ? u : hi; }
    const double span = hi - lo > 1.0e6 ? hi - lo : 1.0e6;
    //                   v0                 dv            hubble   period        sigma      damping  mass         b_turb
    const double runs[][9] = {
        {lo - 0.5 * span, 2.0 * span / 300, 0.0,     0.0,          1.3435e-7, 606.08, 1.6735e-24, 0.0, 0},
        {lo - 0.5 * span, 2.0 * span / 300, 0.0,     0.0,          1.3435e-7, 0.0,    1.6735e-24, 0.0, 0},
        {lo,              span / 64,        2.3e-18, span,         1.3435e-7, 606.08, 1.6735e-24, 2.0e5, 0},
        {hi + 3.0 * span, span / 64,        0.0,     0.0,          1.3435e-7, 0.0,    1.6735e-24, 0.0, 0}, // every core outside: tau is 0
        {lo,              span,             0.0,     0.0,          1.3435e-7, 606.08, 1.6735e-24, 0.0, 0},
    };
    const long long nvel[] = {300, 300, 64, 64, 1};
    for (int r = 0; r < 5; ++r) run(L, runs[r], nvel[r]);
    // a leaf without a line width is named, and nothing is written
    Lists bad = L;
    const size_t at = bad.tgas.size() / 2;
    bad.tgas[at] = -1.0;
    std::vector<double> untouched(64, -7.0);
    bad.off[1] = (long long)bad.tgas.size(); // one line over all segments
    const long long rc2 = sp_lines(1, bad.off.data(), bad.dens.data(), bad.size.data(), bad.tgas.data(), bad.s.data(), bad.u.data(), runs[0], 64,
                                   untouched.data(), nullptr);
    expect(rc2 == (long long)at + 1, "the bad leaf is named", rc2, (double)at + 1, 0);
    for (double v : untouched) expect(v == -7.0, "outputs untouched", 0, v, -7.0);
    if (failures) { std::printf("%d failures\n", failures); return 1; }
    std::printf("sightline spectra under the sanitizers: ok (%lld lines, %lld segments)\n", (long long)L.off.size() - 1, (long long)L.off.back());
    return 0;
}
#endif
