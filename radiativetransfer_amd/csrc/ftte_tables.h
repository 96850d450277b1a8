// ftte_tables.h -- the reference's table mathematics on the host: the dust and photoionisation cross-sections, the stellar
// spectra, the background's group tables, the collisional rate coefficients, the frequency grid and the bins of a population, the
// output cross-sections, the pixel directions and rmax, with the sizes of the tables and FreqBin.  Plain C++: no HIP, nothing of
// the context.  Every expression keeps the reference's operation order; the CPU tests pin the results bit for bit
// (tests/test_abi_and_host.py).
#pragma once

namespace ftte {

constexpr int kFrequencies = 400; // nfreq, stellarBetaTable.f90:14
// The reference writes most constants as default-real literals: they reach the double-precision arithmetic widened from single
// precision (W() in ftte_tables.cpp).
constexpr double kSigmaDustThreshold = (double)5.4116737e-22f;            // what the tabulated dust depth is counted in
constexpr double kKpc = (double)1.e3f * (double)3.08568025e18f;           // definitionsModule.f90:21-22 [cm]

// the rate tables of a population, the tracer's pixels, the escape record of a star
constexpr int kTableDepths = 11;                    // ndepth + 1, definitionsModule.f90:72
constexpr int kTableSize = 11 * 11 * 11 * 11;       // one rate table
constexpr int kMaxPixelLevel = 6;                   // localDefinitions, equiSources.f90:9
constexpr int kPixelCount = 12 * (4096 - 1) / 3;    // pixels of levels 1..6: 12 (4^6 - 1)/3 = 16380
constexpr int kOutputRadii = 7;                     // nradius, equiSources.f90:9
constexpr int kOutputEnergies = 300;                // nenergy, definitionsModule.f90:290
// one star's escape bookkeeping (startNewLongRay, equiSources.f90:3198-3233, 3336-3345): ndotRemaining[7], ndotBoundary[7],
// ndotDust, ndotSpectrum[300]
constexpr int kEscapeRec = 2 * kOutputRadii + 1 + kOutputEnergies;

// One frequency bin of stellarBetaTable as the table kernel needs it
struct FreqBin {
    double dtmp;                 // photons/s in the bin
    double r24, r26, r25, rdust; // sigma(nu)/sigma(threshold) per absorber: multiplies the tabulated depth
    double excess[3];            // (nu - nu_threshold) in erg, per reaction; < 0: below threshold, bin does not count
};

// The three photoionisation cross-sections at nu [eV], zero at and below each threshold: 24 the hydrogenic HI form, 25 the
// hydrogenic HeII form (stellarBetaTable.f90:40-44, :52-56), 26 the HeI fit (:46-50)
struct PhotoSigma { double s24, s25, s26; };
PhotoSigma photo_sigma(double nu);

// dustCrossSection, dustModule.f90:30-73 (SMC branch); a_smc is the Fortran array a_smc(7,5), lambda in micron
double dust_cross_section(double lambda_um, const double *a_smc);
// stellarPopulation, stellarPopulationModule.f90:7-50.  spec is the Fortran array specificLuminosity(nmetal,nspectrum,nwave)
double stellar_population(const double *spec, int nmetal, int nspectrum, int nwave, const double *wavelength, int iSpectrum,
                          double coefSpectrum, int iMetal, double coefMetal, double freq_ev);
// uvbBetaTable(nfreq, freqdel, alpha), uvbBetaTable.f90:3-305: group-averaged cross-sections beta[species HI, HeI, HeII][group],
// photo-rate coefficients ksi[group][24, 25, 26] and heating coefficients gamma[group][HI, HeI, HeII] of the three frequency groups
void uvb_beta_table(int nfreq, double freqdel, const double *alpha, double *beta, double *ksi, double *gamma);
// uniformTable(nfreq, freqdel, alphaQuasar, alphaStellar), uniformTable.f90:1-200: ksi[component quasar, stellar][24, 25, 26] and
// gamma[component][HI, HeI, HeII] of the two power-law components of the uniform background
void uniform_table(int nfreq, double freqdel, double alpha_quasar, double alpha_stellar, double *ksi, double *gamma);
// coll_rates (coll_rates.f:42-150): k1..k6 at temperature T; recombination_type 1 = case A, 2 = case B (definitionsModule.f90:48)
void coll_rates(double T, int recombination_type, double *k);
// k1a..k6a(nratec) as calc_rates.f:324-337 fills them, with the table bounds of equiSources.f90:174-176; k[6][nratec]
void rate_coefficient_tables(int nratec, double temstart, double temend, int recombination_type, double *k, double *logtem0,
                             double *logtem9, double *dlogtem);
// The thirteen cooling coefficients as calc_rates.f:414-544 fills them (flags as compiled, :155), c[13][nratec] in the order of
// equiSources.f90:3975-3987 on the temperature grid of rate_coefficient_tables, and compa (:619).  Case B reads the caller's
// copies of the reference's two data files: mellema[81][2] = columns 1, 3 of HII-ktbetas.tab, gnedin[201][3] = columns 1, 3, 5 of
// cratesHe.res, as the files hold them; case A reads neither.
void cooling_coefficient_tables(int nratec, double temstart, double temend, int recombination_type, const double *mellema,
                                const double *gnedin, double *c, double *compa);
// rmax(1:30), equiSources.f90:296-309
void rmax_table(double *rmax30);

// the frequency grid and the cross-sections on it, stellarBetaTable.f90:27-66: the same for every population
struct FrequencyGrid { double nu[kFrequencies], s24[kFrequencies], s25[kFrequencies], s26[kFrequencies], sd[kFrequencies]; };
void frequency_grid(const double *a_smc, FrequencyGrid &G);
// what every depth tuple needs from a frequency bin of one population, :217-232 and :243-246: bins[kFrequencies - 1]; returns
// totalIntegral
double population_bins(const FrequencyGrid &G, const double *spec, int nmetal, int nspectrum, int nwave, const double *wavelength,
                       int iSpectrum, double coefSpectrum, int iMetal, double coefMetal, FreqBin *bins);
// outputSigma24, 25, 26, Dust on the output energies, sigma[4][kOutputEnergies], stellarBetaTable.f90:119-152 (nenergy = 300 between
// lowerEnergy and upperEnergy, definitionsModule.f90:290-292)
void output_sigma(const double *a_smc, double *sigma);
// Unit vectors of every pixel of levels 1..kMaxPixelLevel, dir[kPixelCount][3].  The reference evaluates cos(phi)*cos(theta),
// sin(phi)*cos(theta), sin(theta) where it needs them (equiSources.f90:2437-2439, :3331-3333); the products are formed here once.
// Returns 0, or what pix2ang_nest refused a pixel with.
int pixel_directions(double *dir);

} // namespace ftte
