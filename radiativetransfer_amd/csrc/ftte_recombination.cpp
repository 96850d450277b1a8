// ftte_recombination.cpp -- the diffuse recombination source of include/ftte.h: the table of ground-state recombination
// coefficients, and the pass that turns the device-resident gas state into the sweep's source function, in place (kernel:
// ftte_recombination.hip; the statement per leaf: ftte_recombination_math.h).
//
// The pass writes where the next sweep reads and nowhere else.  While no emission is in force the source of ftte_ctx::emis is
// nobody's, and the kernel writes straight into it: the way a time loop takes, which switches emission off once a step's sweep
// has carried it (evolution.py).  While one is in force (the caller's own) its values must outlive a refusal, so the kernel writes
// a buffer of the chemistry's (ChemState::ground_out) that is copied into the field once no leaf has failed.  Either way the mode
// changes only then: a refused call leaves the emission state as it was.  MediumField itself is used as it stands.
#include "ftte_context.h"
#include "ftte_recombination.h"

using namespace ftte;

namespace {

int recombination_source(ftte_ctx *c, const double *ksi, const double *share, double *S, bool S_on_device, int64_t *lost, const char *who_)
{
    const std::string who = std::string(who_) + ": ";
    int rc = check_ready(c, false);
    if (rc) return rc;
    ChemState &K = c->chem;
    const GasState &G = c->gas;
    if (!G.ready_with_density(c->ncell)) return fail(c, FTTE_ERR_STATE, who + "no medium with density (ftte_set_medium with rho)");
    if (!K.temperature_set) return fail(c, FTTE_ERR_STATE, who + "no temperature (ftte_set_temperature)");
    if (!K.k) return fail(c, FTTE_ERR_STATE, who + "no rate coefficients (ftte_set_rate_coefficients)");
    if (!K.ground) return fail(c, FTTE_ERR_STATE, who + "no ground-state recombination coefficients (ftte_set_ground_recombination)");
    if (!c->nnu || !c->kappa.source()) return fail(c, FTTE_ERR_STATE, who + "no opacities (ftte_compute_opacities / ftte_set_opacity): they size the emission field");
    if (c->nnu != 3)
        return fail(c, FTTE_ERR_STATE, who + "the opacities have " + std::to_string(c->nnu) + " frequency groups, the recombination source has 3 (ftte_compute_opacities with nnu = 3)");
    if (!ksi || !share) return fail(c, FTTE_ERR_ARG, who + "bad argument");
    for (int i = 0; i < 3; ++i) {
        double row = 0.;
        for (int j = 0; j < 3; ++j) {
            const double s = share[3 * i + j];
            if (!(s >= 0. && s <= 1.)) return fail(c, FTTE_ERR_ARG, who + "share[" + std::to_string(i) + "][" + std::to_string(j) + "] outside [0, 1]");
            row += s;
        }
        if (!(row <= 1.)) return fail(c, FTTE_ERR_ARG, who + "the shares of ion " + std::to_string(i) + " add up to more than 1");
    }
    FTTE_HIP(c, hipSetDevice(c->device));
    if ((rc = wait_sweep(c))) return rc;
    const size_t nc = (size_t)c->ncell;
    const bool in_force = c->emit_mode != 0;
    if (in_force) FTTE_HIP(c, K.ground_out.reserve(3 * nc));
    else {
        FTTE_HIP(c, c->emis.reserve_source(c->kappa.capacity()));
        c->emis.invalidate(); // being written: no copy of it is current, whatever becomes of the pass
    }
    FTTE_HIP(c, K.ground_words.reserve(2));
    unsigned long long words[2] = {~0ull, 0ull};
    FTTE_HIP(c, hipMemcpyAsync(K.ground_words, words, sizeof words, hipMemcpyHostToDevice, c->stream));

    RecombRec R;
    std::memset(&R, 0, sizeof R);
    R.rho = G.field(GasState::kRho); R.HI = G.field(GasState::kHI); R.HeI = G.field(GasState::kHeI); R.HeII = G.field(GasState::kHeII);
    R.logtem = K.logtem; R.g = K.ground;
    R.S = in_force ? K.ground_out.get() : c->emis.source();
    R.first_bad = K.ground_words; R.lost = K.ground_words + 1;
    R.ncell = c->ncell; R.nratec = K.nratec;
    R.logtem0 = K.logtem0; R.logtem9 = K.logtem9; R.dlogtem = K.dlogtem;
    std::memcpy(R.ksi, ksi, sizeof R.ksi);
    std::memcpy(R.share, share, sizeof R.share);
    if (launch_recombination_source(R, c->stream)) return fail(c, FTTE_ERR_NO_DEVICE, who + "kernel launch failed");
    FTTE_HIP(c, hipMemcpyAsync(words, K.ground_words, sizeof words, hipMemcpyDeviceToHost, c->stream));
    FTTE_HIP(c, hipStreamSynchronize(c->stream)); // (the sweep may run on another stream: S has landed)
    if (words[0] != ~0ull)
        return fail(c, FTTE_ERR_RATES, who + "density not positive and finite, or electron density or source function not finite, in cell " +
                                           std::to_string(words[0]) + " (0-based cell-array index)");
    if (in_force) {
        FTTE_HIP(c, hipMemcpyAsync(c->emis.source(), K.ground_out, sizeof(double) * 3 * nc, hipMemcpyDeviceToDevice, c->stream));
        FTTE_HIP(c, hipStreamSynchronize(c->stream));
    }
    c->emis.set();
    c->emit_mode = 2;
    if (S) {
        FTTE_HIP(c, hipMemcpyAsync(S, c->emis.source(), sizeof(double) * 3 * nc, S_on_device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, c->stream));
        FTTE_HIP(c, hipStreamSynchronize(c->stream));
    }
    if (lost) *lost = (int64_t)words[1];
    return FTTE_OK;
}

} // namespace

extern "C" {

int ftte_set_ground_recombination(ftte_ctx *c, int nratec, const double *g)
{
    const std::string who = "ftte_set_ground_recombination: ";
    int rc = check_single(c);
    if (rc) return rc;
    if (nratec < 2 || !g) return fail(c, FTTE_ERR_ARG, who + "bad argument");
    ChemState &K = c->chem;
    if (!K.k) return fail(c, FTTE_ERR_STATE, who + "no rate coefficients (ftte_set_rate_coefficients): the two share one temperature grid");
    if (nratec != K.nratec) return fail(c, FTTE_ERR_ARG, who + "nratec must be that of ftte_set_rate_coefficients, " + std::to_string(K.nratec));
    for (size_t i = 0; i < 3 * (size_t)nratec; ++i)
        if (!(g[i] >= 0.) || !std::isfinite(g[i]))
            return fail(c, FTTE_ERR_ARG, who + "g[" + std::to_string(i / nratec) + "][" + std::to_string(i % nratec) + "] is negative or not finite");
    FTTE_HIP(c, hipSetDevice(c->device));
    FTTE_HIP(c, hipStreamSynchronize(c->stream));
    FTTE_HIP(c, K.ground.reserve(3 * (size_t)nratec));
    hipError_t e = hipMemcpyAsync(K.ground, g, sizeof(double) * 3 * (size_t)nratec, hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream); // (g is the caller's: it may go once this returns)
    if (e != hipSuccess) { K.ground.reset(); return fail(c, FTTE_ERR_NO_DEVICE, who + hipGetErrorString(e)); }
    return FTTE_OK;
}

int ftte_recombination_source(ftte_ctx *c, const double *ksi, const double *share, double *S, int64_t *lost)
{
    return recombination_source(c, ksi, share, S, false, lost, "ftte_recombination_source");
}

int ftte_recombination_source_device(ftte_ctx *c, const double *ksi, const double *share, double *S_dev, int64_t *lost)
{
    return recombination_source(c, ksi, share, S_dev, true, lost, "ftte_recombination_source_device");
}

} // extern "C"
