// ftte_recombination.hip -- the kernel behind ftte_recombination_source (ftte_recombination.cpp): the source function of the diffuse
// recombination radiation of every leaf.  The statement per leaf is ftte_recombination_math.h, compiled here for the device and by
// the tests' host library for the host; the kernel is the loop over the leaves, the leaf's five loads, one call into that header,
// the leaf's three stores and the fold of its two words (ftte_leaf.h).  A stream: 40 bytes read and 24 written per leaf, every
// array in cell-array order with consecutive lanes on consecutive doubles; the two table nodes a leaf gathers stay in cache.
#include <hip/hip_runtime.h>

#include "ftte_leaf.h"
#include "ftte_recombination.h"
#include "ftte_recombination_math.h"

namespace ftte {

// A leaf that does not get through (recomb_source_cell) is noted and writes nothing; the host then leaves the emission state as it was.
__global__ void __launch_bounds__(256) recombination_source_kernel(const RecombRec R)
{
    LeafWords<0, 1> w;
    const ChemTable T = {R.g, R.nratec, R.logtem0, R.logtem9, R.dlogtem};
    FTTE_FOR_LEAVES(c, R.ncell) {
        double S[3], E[3];
        int lost;
        const int ok = recomb_source_cell(&T, R.rho[c], R.logtem[c], R.HI[c], R.HeI[c], R.HeII[c], R.ksi, R.share, S, E, &lost);
        if (!ok) note_bad(w.bad, c);
        else {
            w.sm[0] += (unsigned long long)lost;
            R.S[c] = S[0]; R.S[R.ncell + c] = S[1]; R.S[2 * R.ncell + c] = S[2];
        }
    }
    unsigned long long *const max_to[1] = {nullptr}, *const sum_to[1] = {R.lost};
    fold_words<0, 1>(w, R.first_bad, max_to, sum_to);
}

int launch_recombination_source(const RecombRec &R, hipStream_t stream)
{
    const bool bad = R.nratec < 2 || !R.rho || !R.HI || !R.HeI || !R.HeII || !R.logtem || !R.g || !R.S || !R.first_bad || !R.lost;
    return R.ncell > 0 && bad ? -1 : launch_over_leaves(recombination_source_kernel, R, R.ncell, stream);
}

} // namespace ftte
