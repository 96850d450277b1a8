// ftte_thermochem.hip -- the kernel behind ftte_advance_thermochemistry (ftte_leaf_pass.cpp): species and temperature of every leaf
// advanced together over a time step, each leaf in as many subcycles as its own time scales ask for.  The statement of a cell is
// ftte_thermochem_math.h, compiled here for the device and by the tests' host library for the host; the kernel is the loop over the
// leaves, the leaf's loads, one call into that header, the leaf's stores into the `out` buffers (copied in by the host once no
// leaf has failed), and the fold of its seven words (all of ftte_leaf.h).
#include <hip/hip_runtime.h>

#include "ftte_leaf.h"
#include "ftte_thermochem_math.h"

namespace ftte {

// HI, HeI, HeII and T of every leaf advanced over R.T.dt in at most R.max_subcycles subcycles (thermochem_advance_cell).
// w.mx[]: largest species change, largest T change, largest subcycle count; w.sm[]: bisection steps, subcycles, leaves the cap bounded
__global__ void __launch_bounds__(256) thermochem_advance_kernel(const ThermochemRec R)
{
    const ThermalRec &A = R.T;
    LeafWords<3, 3> w;
    const ChemTable T = {R.k, A.nratec, A.logtem0, A.logtem9, A.dlogtem};
    const ThermalTable C = {A.cool, (long)A.coef_stride, (long)A.node_stride};
    FTTE_FOR_LEAVES(c, A.ncell) {
        double p24, p25, p26, e24, e25, e26, HI, HeI, HeII, T1, logtem1, change, tchange;
        load_point_rates(A.crate, c, 0, p24, p25, p26);
        load_point_rates(A.crate, c, 3, e24, e25, e26);
        unsigned long long steps;
        int subcycles, capped;
        const int ok = thermochem_advance_cell(&A.K, &T, &C, A.rho[c], A.tgas[c], R.logtem[c], A.HI[c], A.HeI[c], A.HeII[c],
                                               chem_cell_volume(A.box, A.level[c], A.n), A.crate != nullptr, p24, p25, p26, e24, e25, e26,
                                               A.run_uvb ? A.J + c : nullptr, A.ncell, R.ksi, R.uniform, A.gamma, A.uniform, A.threshold, A.comp1,
                                               A.comp2, A.hydro ? A.hydro[c] : 0., A.dt, R.eta, R.max_subcycles, A.tmin, A.tmax, &HI, &HeI, &HeII, &T1,
                                               &logtem1, &steps, &subcycles, &capped, &change, &tchange);
        w.sm[0] += steps;
        w.sm[1] += (unsigned long long)subcycles;
        w.sm[2] += (unsigned long long)capped;
        w.mx[2] = (unsigned long long)subcycles > w.mx[2] ? (unsigned long long)subcycles : w.mx[2];
        R.subcycles[c] = subcycles;
        if (!ok) note_bad(w.bad, c);
        else {
            note_change(w.mx[0], change);
            note_change(w.mx[1], tchange);
            R.HI_out[c] = HI; R.HeI_out[c] = HeI; R.HeII_out[c] = HeII;
            A.out0[c] = T1; A.out1[c] = logtem1;
        }
    }
    unsigned long long *const max_to[3] = {A.max_change, R.max_tchange, R.sub_max}, *const sum_to[3] = {A.steps, R.sub_sum, R.capped};
    fold_words<3, 3>(w, A.first_bad, max_to, sum_to);
}

int launch_thermochem_advance(const ThermochemRec &R, hipStream_t stream)
{
    const ThermalRec &A = R.T;
    const bool bad = A.nratec < 2 || !A.cool || !R.k || !R.logtem || !A.out0 || !A.out1 || !R.HI_out || !R.HeI_out || !R.HeII_out || !R.subcycles ||
                     !R.max_tchange || !R.sub_sum || !R.sub_max || !R.capped || R.max_subcycles < 1 || !(R.eta >= 0.) || !(A.dt > 0.) ||
                     !(A.tmin > 0.) || !(A.tmax > A.tmin);
    return A.ncell > 0 && bad ? -1 : launch_over_leaves(thermochem_advance_kernel, R, A.ncell, stream);
}

} // namespace ftte
