// fit_tables.h -- what the stand-alone host checks of the per-leaf updates share (thermochem_check.cpp, leaf_pass_check.cpp): rate and
// cooling tables of the usual shape, and a random sequence that is the same everywhere.  tests/host/ only.
#pragma once
#include <cmath>
#include <cstdint>
#include <vector>

// tables of the usual shape (the fits of thermal_check.cpp and chem_advance_check.cpp's kind: Black 1981, MNRAS 197, 553; Cen
// 1992, ApJS 78, 341), only to have rows that span what real ones span
inline void fill_tables(int nratec, double logtem0, double dlogtem, std::vector<double> &k, std::vector<double> &c)
{
    k.assign(6 * (size_t)nratec, 0.);
    c.assign(13 * (size_t)nratec, 0.);
    for (int i = 0; i < nratec; ++i) {
        const double T = std::exp(logtem0 + i * dlogtem), s = std::sqrt(T), f = 1. / (1. + std::sqrt(T / 1e5));
        const double kr[6] = {5.85e-11 * s * std::exp(-157809.1 / T) * f, 8.4e-11 / s * std::pow(T / 1e3, -0.2) / (1. + std::pow(T / 1e6, 0.7)),
                              2.38e-11 * s * std::exp(-285335.4 / T) * f,
                              1.5e-10 * std::pow(T, -0.6353) + 1.9e-3 * std::pow(T, -1.5) * std::exp(-470000. / T) * (1. + 0.3 * std::exp(-94000. / T)),
                              5.68e-12 * s * std::exp(-631515. / T) * f, 3.36e-10 / s * std::pow(T / 1e3, -0.2) / (1. + std::pow(T / 1e6, 0.7))};
        for (int r = 0; r < 6; ++r) k[(size_t)r * nratec + i] = kr[r];
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
