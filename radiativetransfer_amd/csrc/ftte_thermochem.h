// ftte_thermochem.h -- the launch record and the launch wrapper of ftte_thermochem.hip: species and temperature of every leaf
// advanced together over a time step, each leaf in subcycles of its own (ftte_thermochem_math.h).  Asynchronous on `stream`;
// returns 0, -1 bad argument, -2 launch failure.
#pragma once
#include "ftte_thermal.h"

namespace ftte {

// The thermal advance's record (tgas, the species, crate -- the packed point-source rates, krate24..26 at +0..+2 --, J, hydro, the
// cooling table, gamma, uniform, the clip, dt; out0 = T, out1 = logtem; first_bad, max_change = the species', steps) and what
// the chemistry adds to it
struct ThermochemRec {
    ThermalRec T;
    const double *logtem;      // per leaf: the stored logarithm the first subcycle's chemistry reads
    const double *k;           // [6][nratec] rate coefficients k1a..k6a
    double *HI_out, *HeI_out, *HeII_out;
    int32_t *subcycles;        // per leaf: the subcycles it took
    double ksi[9];             // [group][ksi24, ksi25, ksi26]
    double uniform[3];         // the uniform background's ionisation rates, per reaction
    double eta;
    int32_t max_subcycles;
    // bits of the largest |T1 - T0| / T0, sum of the subcycles, largest subcycle count of a leaf, leaves the cap bounded
    unsigned long long *max_tchange, *sub_sum, *sub_max, *capped;
};

int launch_thermochem_advance(const ThermochemRec &R, hipStream_t stream);

} // namespace ftte
