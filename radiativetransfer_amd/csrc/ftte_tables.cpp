// ftte_tables.cpp -- the reference's table mathematics on the host.  See ftte_tables.h.
#include "ftte_tables.h"

#include <cmath>
#include <cstddef>
#include <vector>

#include "ftte_chem_math.h"
#include "ftte_geometry.h"

namespace ftte {

namespace {

// The reference writes most constants as default-real literals; they reach the double-precision arithmetic widened
// from single precision.  W() spells that out.
#define W(x) ((double)(x##f))

const double kHydrogen = W(13.598), kHeI = W(24.587), kHeII = W(54.418); // definitionsModule.f90:30-32
inline double c_light() { return W(2.99792458e10); }
inline double ev_to_erg() { return 1.60217646e-12; }
inline double ev_to_hz() { return 1.60217646e-12 / W(6.6260693e-27); }
inline double pi_ref() { return FTTE_PI; }

inline double pow4(double x) { return x * x * x * x; }

// hydrogenic photoionisation cross-section above threshold, stellarBetaTable.f90:40-44 and :52-56
inline double hydrogenic(double sigma0, double threshold, double nu)
{
    const double dum = std::sqrt(nu / threshold - 1);
    return sigma0 * pow4(threshold / nu) * std::exp(4.0 - 4.0 * std::atan(dum) / dum) / (1 - std::exp(-2.0 * pi_ref() / dum));
}

inline double powi_left(double x, int n)
{
    double r = x;
    for (int i = 1; i < n; ++i) r = r * x;
    return r;
}

} // namespace

PhotoSigma photo_sigma(double nu)
{
    PhotoSigma S;
    S.s24 = nu > kHydrogen ? hydrogenic(FTTE_SIGMA_HI, kHydrogen, nu) : 0.0;
    S.s25 = nu > kHeII ? hydrogenic(FTTE_SIGMA_HEII, kHeII, nu) : 0.0;
    S.s26 = nu > kHeI ? FTTE_SIGMA_HEI * (W(1.66) * std::pow(nu / kHeI, (double)(-2.05f)) - W(0.66) * std::pow(nu / kHeI, (double)(-3.05f)))
                      : 0.0;
    return S;
}

double dust_cross_section(double lambda_um, const double *a_smc)
{
    double sigma = 0.0;
    for (int i = 0; i < 7; ++i) {
        // a_smc(i,1:5): lambda_i, a_i, b_i, p_i, q_i
        const double l = a_smc[i], a = a_smc[i + 7], b = a_smc[i + 14], p = a_smc[i + 21], q = a_smc[i + 28];
        const double x = lambda_um / l;
        sigma = sigma + a / (std::pow(x, p) + std::pow(x, -q) + b);
    }
    return W(1.1) * sigma * (double)0.9210340372f;
}

double stellar_population(const double *spec, int nmetal, int nspectrum, int nwave, const double *wavelength, int iSpectrum,
                          double cS, int iMetal, double cM, double freq_ev)
{
    auto SL = [&](int m, int s, int w) { return spec[(size_t)(m - 1) + (size_t)nmetal * ((size_t)(s - 1) + (size_t)nspectrum * (size_t)(w - 1))]; };
    const double lam = c_light() / (freq_ev * ev_to_hz());
    int iw = 1;
    while (iw + 1 < nwave && lam > wavelength[iw]) ++iw;
    double cw = (lam - wavelength[iw - 1]) / (wavelength[iw] - wavelength[iw - 1]);
    cw = std::fmin(std::fmax(0.0, cw), 1.0);
    const double sp1 = cS * ((1.0 - cw) * SL(iMetal, iSpectrum + 1, iw) + cw * 1.0 * SL(iMetal, iSpectrum + 1, iw + 1)) +
                       (1.0 - cS) * ((1.0 - cw) * SL(iMetal, iSpectrum, iw) + cw * SL(iMetal, iSpectrum, iw + 1));
    const double sp2 = cS * ((1.0 - cw) * SL(iMetal + 1, iSpectrum + 1, iw) + cw * 1.0 * SL(iMetal + 1, iSpectrum + 1, iw + 1)) +
                       (1.0 - cS) * ((1.0 - cw) * SL(iMetal + 1, iSpectrum, iw) + cw * SL(iMetal + 1, iSpectrum, iw + 1));
    double sp = (1.0 - cM) * sp1 + cM * sp2;
    const double nu_hz = freq_ev * ev_to_hz();
    sp = std::pow(10.0, sp) / W(1.e-8) * c_light() / (nu_hz * nu_hz);
    return sp;
}

void uvb_beta_table(int nfreq, double freqdel, const double *alpha, double *beta, double *ksi, double *gamma)
{
    // uvbBetaTable.f90:40-66: the frequency grid and the three cross-sections on it
    std::vector<double> nu(nfreq), s24(nfreq), s25(nfreq), s26(nfreq);
    for (int i = 0; i < nfreq; ++i) {
        nu[i] = std::pow(10.0, (double)i * freqdel);
        const PhotoSigma S = photo_sigma(nu[i]);
        s24[i] = S.s24; s25[i] = S.s25; s26[i] = S.s26;
    }
    const double nu1 = kHydrogen, nu2 = kHeI, nu3 = kHeII;
    const double lo[3] = {nu1, nu2, nu3}, hi[3] = {nu2, nu3, HUGE_VAL};
    double b[3][3] = {}, k[3][3] = {}, g[3][3] = {}; // [group][24, 25, 26] / [group][HI, HeI, HeII]
    for (int i = 1; i < nfreq; ++i) { // :171-252
        const double freq = nu[i], delta_nu = nu[i] - nu[i - 1];
        for (int q = 0; q < 3; ++q) {
            if (!(freq >= lo[q] && freq <= hi[q])) continue;
            const double dtmp = std::pow(freq / lo[q], -alpha[q]) * delta_nu;
            const double over = dtmp * ev_to_hz() / (freq * ev_to_erg());
            b[q][0] = b[q][0] + dtmp * s24[i]; b[q][1] = b[q][1] + dtmp * s25[i]; b[q][2] = b[q][2] + dtmp * s26[i];
            k[q][0] = k[q][0] + over * s24[i]; k[q][1] = k[q][1] + over * s25[i]; k[q][2] = k[q][2] + over * s26[i];
            g[q][0] = g[q][0] + over * (freq - nu1) * ev_to_erg() * s24[i];
            if (q >= 1) g[q][1] = g[q][1] + over * (freq - nu2) * ev_to_erg() * s26[i];
            if (q == 2) g[q][2] = g[q][2] + over * (freq - nu3) * ev_to_erg() * s25[i];
        }
    }
    // :254-296: beta is normalised by the group's energy shape
    const double shape[3] = {(1. - std::pow(nu2 / nu1, 1. - alpha[0])) / (alpha[0] - 1.),
                             (1. - std::pow(nu3 / nu2, 1. - alpha[1])) / (alpha[1] - 1.), 1. / (alpha[2] - 1.)};
    for (int q = 0; q < 3; ++q) {
        const double energy_shape = shape[q] * lo[q];
        // out: beta[species HI, HeI, HeII][group]; ksi[group][24, 25, 26]; gamma[group][HI, HeI, HeII]
        beta[0 * 3 + q] = b[q][0] / energy_shape;
        beta[1 * 3 + q] = b[q][2] / energy_shape;
        beta[2 * 3 + q] = b[q][1] / energy_shape;
        for (int r = 0; r < 3; ++r) { ksi[q * 3 + r] = k[q][r]; gamma[q * 3 + r] = g[q][r]; }
    }
}

void uniform_table(int nfreq, double freqdel, double alpha_quasar, double alpha_stellar, double *ksi, double *gamma)
{
    const double nu1 = kHydrogen, nu2 = kHeI, nu3 = kHeII;
    const double alpha[2] = {alpha_quasar, alpha_stellar};
    for (int q = 0; q < 6; ++q) ksi[q] = gamma[q] = 0.0;
    double prev = 0.0;
    for (int i = 0; i < nfreq; ++i) {
        const double nu = std::pow(10.0, (double)i * freqdel);
        const PhotoSigma S = photo_sigma(nu);
        const double s24 = S.s24, s25 = S.s25, s26 = S.s26;
        if (i >= 1) { // uniformTable.f90:136-190
            const double delta_nu = nu - prev;
            for (int c = 0; c < 2; ++c) {
                const double dtmp = std::pow(nu / nu1, -alpha[c]) * delta_nu;
                const double over = dtmp * ev_to_hz() / (nu * ev_to_erg());
                if (nu >= nu1) {
                    ksi[3 * c + 0] = ksi[3 * c + 0] + over * s24;
                    ksi[3 * c + 1] = ksi[3 * c + 1] + over * s25;
                    ksi[3 * c + 2] = ksi[3 * c + 2] + over * s26;
                    gamma[3 * c + 0] = gamma[3 * c + 0] + over * (nu - nu1) * ev_to_erg() * s24;
                }
                if (nu >= nu2) gamma[3 * c + 1] = gamma[3 * c + 1] + over * (nu - nu2) * ev_to_erg() * s26;
                if (nu >= nu3) gamma[3 * c + 2] = gamma[3 * c + 2] + over * (nu - nu3) * ev_to_erg() * s25;
            }
        }
        prev = nu;
    }
}

void coll_rates(double T, int recombination_type, double *k)
{
    // coll_rates.f:62-150 (fits of Abel et al. 1997 and Hui & Gnedin 1997); its literals are single precision
    const double T_eV = T / W(11605.);
    const double L = std::log(T_eV);
    if (T_eV > W(0.8)) {
        k[0] = std::exp(W(-32.71396786375) + W(13.53655609057) * L - W(5.739328757388) * powi_left(L, 2) + W(1.563154982022) * powi_left(L, 3) -
                        W(0.2877056004391) * powi_left(L, 4) + W(0.03482559773736999) * powi_left(L, 5) - W(0.00263197617559) * powi_left(L, 6) +
                        W(0.0001119543953861) * powi_left(L, 7) - W(2.039149852002e-6) * powi_left(L, 8));
        k[2] = std::exp(W(-44.09864886561001) + W(23.91596563469) * L - W(10.75323019821) * powi_left(L, 2) + W(3.058038757198) * powi_left(L, 3) -
                        W(0.5685118909884001) * powi_left(L, 4) + W(0.06795391233790001) * powi_left(L, 5) -
                        W(0.005009056101857001) * powi_left(L, 6) + W(0.0002067236157507) * powi_left(L, 7) -
                        W(3.649161410833e-6) * powi_left(L, 8));
        k[4] = std::exp(W(-68.71040990212001) + W(43.93347632635) * L - W(18.48066993568) * powi_left(L, 2) + W(4.701626486759002) * powi_left(L, 3) -
                        W(0.7692466334492) * powi_left(L, 4) + W(0.08113042097303) * powi_left(L, 5) - W(0.005324020628287001) * powi_left(L, 6) +
                        W(0.0001975705312221) * powi_left(L, 7) - W(3.165581065665e-6) * powi_left(L, 8));
    } else {
        k[0] = k[2] = k[4] = W(1.0e-20);
    }
    const double kb = 1.3806503e-16, ev = 1.60217646e-12;
    if (recombination_type == 1) { // case A
        if (T_eV > W(0.8))
            k[3] = W(1.54e-9) * (1. + W(0.3) / std::exp(W(8.099328789667) / T_eV)) / (std::exp(W(40.49664394833662) / T_eV) * std::pow(T_eV, W(1.5))) +
                   W(3.92e-13) / std::pow(T_eV, W(0.6353));
        else k[3] = W(3.92e-13) / std::pow(T_eV, W(0.6353));
        if (T > W(5500.0))
            k[1] = std::exp(W(-28.61303380689232) - W(0.7241125657826851) * L - W(0.02026044731984691) * powi_left(L, 2) -
                            W(0.002380861877349834) * powi_left(L, 3) - W(0.0003212605213188796) * powi_left(L, 4) -
                            W(0.00001421502914054107) * powi_left(L, 5) + W(4.989108920299513e-6) * powi_left(L, 6) +
                            W(5.755614137575758e-7) * powi_left(L, 7) - W(1.856767039775261e-8) * powi_left(L, 8) -
                            W(3.071135243196595e-9) * powi_left(L, 9));
        else k[1] = k[3];
        k[5] = W(3.36e-10) / std::sqrt(T) / std::pow(T / W(1.e3), W(0.2)) / (1. + std::pow(T / W(1.e6), W(0.7)));
    } else { // case B
        double tmp = (double)(2.f * 24.587f) * ev / (kb * T);
        k[3] = W(1.26e-14) * (std::sqrt(tmp) * std::sqrt(std::sqrt(tmp))); // tmp**0.750 as the reference's compiler forms it
        tmp = (double)(2.f * 13.598f) * ev / (kb * T);
        k[1] = W(2.753e-14) * std::pow(tmp, W(1.500)) / std::pow(1. + std::pow(tmp / W(2.740), W(0.407)), W(2.242));
        tmp = (double)(2.f * 54.418f) * ev / (kb * T);
        k[5] = (double)(2.f * 2.753e-14f) * std::pow(tmp, W(1.500)) / std::pow(1. + std::pow(tmp / W(2.740), W(0.407)), W(2.242));
    }
}

void rate_coefficient_tables(int nratec, double temstart, double temend, int recombination_type, double *k, double *logtem0,
                             double *logtem9, double *dlogtem)
{
    *logtem0 = std::log(temstart);
    *logtem9 = std::log(temend);
    *dlogtem = (std::log(temend) - std::log(temstart)) / (double)(float)(nratec - 1);
    for (int i = 1; i <= nratec; ++i) { // calc_rates.f:324-337
        const double ttt = std::exp(std::log(temstart) + (double)(float)(i - 1) * *dlogtem);
        double six[6];
        coll_rates(ttt, recombination_type, six);
        for (int r = 0; r < 6; ++r) k[(size_t)r * nratec + (i - 1)] = six[r];
    }
}

namespace {

// one case-B entry: 0 outside the file's temperatures, else 10.** the linear interpolation in log10 T (calc_rates.f:471-483,
// :492-508); n nodes t[] (log10 T) and v[] (log10 of the coefficient).  At log10ttt == t(1) the reference's search stops at j = 1 and
// reads t(0); here that point takes the first interval, whose weight there is 0.
double case_b_entry(double log10ttt, const double *t, const double *v, int n)
{
    if (log10ttt < t[0] || log10ttt > t[n - 1]) return 0.;
    int j = 1; // 1-based, as the reference counts
    while (log10ttt > t[j - 1]) ++j;
    if (j < 2) j = 2;
    return std::pow(10., (log10ttt - t[j - 2]) / (t[j - 1] - t[j - 2]) * (v[j - 1] - v[j - 2]) + v[j - 2]);
}

} // namespace

void cooling_coefficient_tables(int nratec, double temstart, double temend, int recombination_type, const double *mellema,
                                const double *gnedin, double *c, double *compa)
{
    const double dlogtem = (std::log(temend) - std::log(temstart)) / (double)(float)(nratec - 1);
    const double lhuge = std::log(1.0e30); // dlog(dhuge), calc_rates.f:160
    std::vector<double> tM, cM, tG, c2G, c3G;
    if (recombination_type != 1) { // :397-411: Mellema's file holds log10 values, Gnedin's the values themselves
        for (int i = 0; i < 81; ++i) { tM.push_back(mellema[2 * i]); cM.push_back(mellema[2 * i + 1]); }
        for (int i = 0; i < 201; ++i) {
            tG.push_back(std::log10(gnedin[3 * i])); c2G.push_back(std::log10(gnedin[3 * i + 1])); c3G.push_back(std::log10(gnedin[3 * i + 2]));
        }
    }
    for (int i = 1; i <= nratec; ++i) { // :414-544
        const double ttt = std::exp(std::log(temstart) + (double)(float)(i - 1) * dlogtem), log10ttt = std::log10(ttt);
        double six[6], *at = c + (i - 1);
        const size_t row = (size_t)nratec;
        coll_rates(ttt, recombination_type, six);
        const double soft = 1. + std::sqrt(ttt / 1.0e5);
        // a) collisional excitations, :423-428
        at[0 * row] = 7.5e-19 * std::exp(-std::fmin(lhuge, W(118348.) / ttt)) / soft;
        at[1 * row] = 9.1e-27 * std::exp(-std::fmin(lhuge, W(13179.) / ttt)) * std::pow(ttt, W(-0.1687)) / soft;
        at[2 * row] = 5.54e-17 * std::exp(-std::fmin(lhuge, W(473638.) / ttt)) * std::pow(ttt, W(-0.397)) / soft;
        // b) collisional ionisations, :446-453
        at[3 * row] = 2.18e-11 * six[0];
        at[4 * row] = 3.94e-11 * six[2];
        at[5 * row] = 5.01e-27 * std::pow(ttt, W(-0.1687)) / soft * std::exp(-std::fmin(lhuge, W(55338.) / ttt));
        at[6 * row] = 8.72e-11 * six[4];
        // c) recombinations, :467-515
        if (recombination_type == 1) {
            at[7 * row] = 8.70e-27 * std::sqrt(ttt) * std::pow(ttt / W(1000.0), W(-0.2)) / (W(1.0) + std::pow(ttt / 1.0e6, W(0.7)));
            at[8 * row] = 1.55e-26 * std::pow(ttt, W(0.3647));
            at[10 * row] = 3.48e-26 * std::sqrt(ttt) * std::pow(ttt / W(1000.0), W(-0.2)) / (W(1.0) + std::pow(ttt / 1.0e6, W(0.7)));
        } else {
            at[7 * row] = case_b_entry(log10ttt, tM.data(), cM.data(), 81);
            at[8 * row] = case_b_entry(log10ttt, tG.data(), c2G.data(), 201);
            at[10 * row] = case_b_entry(log10ttt, tG.data(), c3G.data(), 201);
        }
        at[9 * row] = 1.24e-13 * std::pow(ttt, W(-1.5)) * std::exp(-std::fmin(lhuge, W(470000.) / ttt)) *
                      (W(1.) + W(0.3) * std::exp(-std::fmin(lhuge, W(94000.) / ttt)));
        // d) bremsstrahlung, :527-528
        const double off = W(5.5) - log10ttt;
        at[11 * row] = 1.43e-27 * std::sqrt(ttt) * (W(1.1) + W(0.34) * std::exp(-(off * off) / W(3.0)));
        // HI line excitation, :543-544
        const double tmp = (double)(2.f * 13.598f) * 1.60217646e-12 / (1.3806503e-16 * ttt);
        at[12 * row] = W(7.5e-19) * std::exp(W(-0.75) * tmp / W(2.)) / (W(1.) + std::sqrt(ttt / W(1.e5)));
    }
    *compa = 5.65e-36; // :619
}

void rmax_table(double *rmax30)
{
    for (int ir = 1; ir <= 30; ++ir) {
        const float v = std::sqrt(3.f) * (std::sqrt(0.5f * std::pow(4.f, (float)(ir - 1)) - 1.f / 12.f) + 0.5f);
        rmax30[ir - 1] = (double)v / 2.0;
    }
}

void frequency_grid(const double *a_smc, FrequencyGrid &G)
{
    const double freqdel = W(0.02);
    for (int i = 0; i < kFrequencies; ++i) {
        G.nu[i] = std::pow(10.0, (double)i * freqdel);
        const double lambda = c_light() / (G.nu[i] * ev_to_hz()) * W(1.e8); // Angstrom
        G.sd[i] = dust_cross_section(lambda / W(1.e4), a_smc) * W(1.e-22);
        const PhotoSigma S = photo_sigma(G.nu[i]);
        G.s24[i] = S.s24; G.s25[i] = S.s25; G.s26[i] = S.s26;
    }
}

double population_bins(const FrequencyGrid &G, const double *spec, int nmetal, int nspectrum, int nwave, const double *wavelength,
                       int iSpectrum, double cS, int iMetal, double cM, FreqBin *bins)
{
    double total = 0.0;
    const double thr[3] = {kHydrogen, kHeI, kHeII};
    for (int i = 1; i < kFrequencies; ++i) {
        const double freq = G.nu[i], delta_nu = G.nu[i] - G.nu[i - 1];
        const double lum = stellar_population(spec, nmetal, nspectrum, nwave, wavelength, iSpectrum, cS, iMetal, cM, freq);
        FreqBin &B = bins[i - 1];
        B.dtmp = lum / (freq * ev_to_erg()) * delta_nu * ev_to_hz();
        if (freq >= kHydrogen) total = total + B.dtmp;
        B.r24 = G.s24[i] / FTTE_SIGMA_HI;
        B.r26 = G.s26[i] / FTTE_SIGMA_HEI;
        B.r25 = G.s25[i] / FTTE_SIGMA_HEII;
        B.rdust = G.sd[i] / kSigmaDustThreshold;
        for (int r = 0; r < 3; ++r) B.excess[r] = freq >= thr[r] ? (freq - thr[r]) * ev_to_erg() : -1.0;
    }
    return total;
}

void output_sigma(const double *a_smc, double *sigma)
{
    const double lower = kHydrogen, upper = W(10.) * kHydrogen; // lowerEnergy, upperEnergy
    for (int ie = 1; ie <= kOutputEnergies; ++ie) {
        // float(ienergy-1)/float(nenergy-1) is a single-precision quotient, :122
        const double freq = lower * std::exp((double)((float)(ie - 1) / (float)(kOutputEnergies - 1)) * (std::log(upper) - std::log(lower)));
        const double lambda = c_light() / (freq * ev_to_hz()) * W(1.e8);
        const PhotoSigma S = photo_sigma(freq);
        sigma[3 * kOutputEnergies + ie - 1] = dust_cross_section(lambda / W(1.e4), a_smc) * W(1.e-22);
        sigma[0 * kOutputEnergies + ie - 1] = freq == kHydrogen ? FTTE_SIGMA_HI : S.s24; // here the threshold itself counts
        sigma[1 * kOutputEnergies + ie - 1] = S.s25;
        sigma[2 * kOutputEnergies + ie - 1] = S.s26;
    }
}

int pixel_directions(double *dir)
{
    size_t at = 0;
    for (int L = 1; L <= kMaxPixelLevel; ++L) {
        const int nside = 1 << (L - 1);
        const int64_t npix = (int64_t)12 * nside * nside;
        for (int64_t ip = 0; ip < npix; ++ip, ++at) {
            double phi, theta;
            if (const int rc = pix2ang_nest(nside, ip, &phi, &theta)) return rc;
            dir[3 * at + 0] = std::cos(phi) * std::cos(theta);
            dir[3 * at + 1] = std::sin(phi) * std::cos(theta);
            dir[3 * at + 2] = std::sin(theta);
        }
    }
    return 0;
}

} // namespace ftte
