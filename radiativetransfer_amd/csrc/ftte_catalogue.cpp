// ftte_catalogue.cpp -- the C ABI of the star catalogue: ftte_star_catalogue (the launches of ftte_catalogue.hip behind their
// checks), ftte_star_sources (the sources of the last catalogue, with their host cells' abun2), and on the host alone
// ftte_star_populations (the metallicity bracket and the population slots) and ftte_cell_position (a leaf's call sequence).  The
// rules themselves are in ftte_catalogue.h.
#include "ftte_context.h"

using namespace ftte;

namespace ftte {

long long catalogue_phase_ns(const StarCatalogue &K, int phase)
{
    if (K.sources() < 0 || K.stars() == 0 || phase < 0 || phase > 3 || (phase == 3 && !K.emitted)) return -1;
    const int a = phase == 3 ? 4 : phase;
    float ms = 0.f;
    if (hipEventElapsedTime(&ms, K.ev[a], K.ev[a + 1]) != hipSuccess) return -1;
    return (long long)((double)ms * 1.0e6);
}

} // namespace ftte

extern "C" {

int ftte_star_catalogue(ftte_ctx *c, int64_t nstars, const double *xyz, const double lo[3], const double hi[3], const int32_t *weight,
                        int64_t *star_cell, int64_t *nsrc, int64_t *outside)
{
    const std::string who = "ftte_star_catalogue: ";
    int rc = check_ready(c, false);
    if (rc) return rc;
    if (nstars < 0 || (nstars > 0 && !xyz) || !lo || !hi) return fail(c, FTTE_ERR_ARG, who + "bad argument");
    if (nstars > 0x7fffffffLL) return fail(c, FTTE_ERR_ARG, who + "more than 2^31 - 1 stars");
    for (int q = 0; q < 3; ++q)
        if (!std::isfinite(lo[q]) || !std::isfinite(hi[q]) || !(hi[q] > lo[q]))
            return fail(c, FTTE_ERR_ARG, who + "the box needs finite lo < hi, axis " + std::to_string(q));
    if (weight) {
        int64_t sum = 0; // the reference's weight is a default integer, and so are count and first on the device
        for (int64_t s = 0; s < nstars; ++s) {
            if (weight[s] < 0) return fail(c, FTTE_ERR_ARG, who + "negative weight of star " + std::to_string(s));
            sum += weight[s];
            if (sum > 0x7fffffffLL) return fail(c, FTTE_ERR_ARG, who + "the weights exceed 2^31 - 1 in sum at star " + std::to_string(s));
        }
    }
    StarCatalogue &K = c->catalogue;
    if (nstars == 0) {
        K.begin();
        K.made(0, 0);
        if (nsrc) *nsrc = 0;
        if (outside) *outside = 0;
        return FTTE_OK;
    }

    FTTE_HIP(c, hipSetDevice(c->device));
    FTTE_HIP(c, c->dtree.ensure(c->stream, c->tree));
    const size_t ns = (size_t)nstars, nc = (size_t)c->ncell;
    const int64_t nblock = (c->ncell + kCatTile - 1) / kCatTile;
    if (nblock > 0x7ffffffeLL) return fail(c, FTTE_ERR_UNSUPPORTED, who + "too many leaves");
    K.begin();
    FTTE_HIP(c, K.xyz.reserve(3 * ns));
    if (weight) FTTE_HIP(c, K.weight.reserve(ns));
    FTTE_HIP(c, K.star_cell.reserve(ns));
    FTTE_HIP(c, K.count.reserve(nc));
    FTTE_HIP(c, K.first.reserve(nc));
    FTTE_HIP(c, K.block_total.reserve((size_t)nblock + 1));
    FTTE_HIP(c, K.outside.reserve(1));
    if ((rc = upload(c, K.xyz, xyz, sizeof(double) * 3 * ns))) return rc;
    if (weight && (rc = upload(c, K.weight, weight, sizeof(int32_t) * ns))) return rc;
    FTTE_HIP(c, hipMemsetAsync(K.count, 0, sizeof(int32_t) * nc, c->stream));
    FTTE_HIP(c, hipMemsetD32Async((hipDeviceptr_t)K.first.get(), kCatNoStar, nc, c->stream));
    FTTE_HIP(c, hipMemsetAsync(K.outside, 0, sizeof(unsigned long long), c->stream));

    LocateRecT<NodeRec> L;
    L.xyz = K.xyz; L.weight = weight ? K.weight.get() : nullptr; L.node = c->dtree.nodes();
    L.star_cell = K.star_cell; L.count = K.count; L.first = K.first; L.outside = K.outside;
    for (int q = 0; q < 3; ++q) { L.lo[q] = lo[q]; L.hi[q] = hi[q]; }
    L.n = c->n; L.nstars = (int32_t)nstars;
    CompactRec R;
    R.count = K.count; R.first = K.first; R.block_total = K.block_total;
    R.src_cell = nullptr; R.src_weight = nullptr; R.src_first = nullptr;
    R.ncell = c->ncell; R.nblock = (int32_t)nblock;
    for (Event &e : K.ev) FTTE_HIP(c, e.create());
    int lrc = 0;
    FTTE_HIP(c, hipEventRecord(K.ev[0], c->stream));
    lrc |= launch_star_locate(L, c->stream.get());
    FTTE_HIP(c, hipEventRecord(K.ev[1], c->stream));
    lrc |= launch_compact_count(R, c->stream.get());
    FTTE_HIP(c, hipEventRecord(K.ev[2], c->stream));
    lrc |= launch_compact_scan(R, c->stream.get());
    FTTE_HIP(c, hipEventRecord(K.ev[3], c->stream));
    if (lrc) return fail(c, FTTE_ERR_NO_DEVICE, who + "kernel launch failed");
    int32_t total = 0;
    unsigned long long out = 0;
    FTTE_HIP(c, hipMemcpyAsync(&total, K.block_total + nblock, sizeof total, hipMemcpyDeviceToHost, c->stream));
    FTTE_HIP(c, hipMemcpyAsync(&out, K.outside, sizeof out, hipMemcpyDeviceToHost, c->stream));
    FTTE_HIP(c, hipStreamSynchronize(c->stream));
    if (total > 0) {
        FTTE_HIP(c, K.src_cell.reserve((size_t)total));
        FTTE_HIP(c, K.src_weight.reserve((size_t)total));
        FTTE_HIP(c, K.src_first.reserve((size_t)total));
        R.src_cell = K.src_cell; R.src_weight = K.src_weight; R.src_first = K.src_first;
        FTTE_HIP(c, hipEventRecord(K.ev[4], c->stream));
        if (launch_compact_emit(R, c->stream.get())) return fail(c, FTTE_ERR_NO_DEVICE, who + "kernel launch failed");
        FTTE_HIP(c, hipEventRecord(K.ev[5], c->stream));
    }
    K.emitted = total > 0;
    if (star_cell) {
        if ((rc = download(c, star_cell, K.star_cell, sizeof(int64_t) * ns))) return rc;
    } else FTTE_HIP(c, hipStreamSynchronize(c->stream));
    K.made(nstars, total);
    if (nsrc) *nsrc = total;
    if (outside) *outside = (int64_t)out;
    return FTTE_OK;
}

int ftte_star_sources(ftte_ctx *c, int64_t nsrc, int64_t *src_cell, int32_t *src_weight, double *src_ndot, int64_t *src_first_star,
                      double *src_abun2)
{
    const std::string who = "ftte_star_sources: ";
    int rc = check_ready(c, false);
    if (rc) return rc;
    StarCatalogue &K = c->catalogue;
    if (K.sources() < 0) return fail(c, FTTE_ERR_STATE, who + "no catalogue: call ftte_star_catalogue first");
    if (nsrc != K.sources())
        return fail(c, FTTE_ERR_ARG, who + "nsrc is not the number of sources of the last ftte_star_catalogue (" + std::to_string(K.sources()) + ")");
    if (src_abun2 && !c->gas.ready_with_abundance(c->ncell))
        return fail(c, FTTE_ERR_STATE, who + "no medium with abun2 (ftte_set_medium with abun2)");
    if (!nsrc) return FTTE_OK;
    FTTE_HIP(c, hipSetDevice(c->device));
    const size_t ns = (size_t)nsrc;
    if (src_cell && (rc = download(c, src_cell, K.src_cell, sizeof(int64_t) * ns))) return rc;
    if (src_first_star && (rc = download(c, src_first_star, K.src_first, sizeof(int64_t) * ns))) return rc;
    if (src_weight || src_ndot) {
        std::vector<int32_t> local;
        int32_t *w = src_weight;
        if (!w) { local.resize(ns); w = local.data(); }
        if ((rc = download(c, w, K.src_weight, sizeof(int32_t) * ns))) return rc;
        if (src_ndot)
            for (size_t s = 0; s < ns; ++s) src_ndot[s] = (double)(float)w[s]; // ndot1 = float(currentStar%weight), :1306
    }
    if (src_abun2) {
        FTTE_HIP(c, K.src_abun2.reserve(ns));
        if (launch_gather(c->gas.field(GasState::kAbun2), K.src_cell, (int)nsrc, K.src_abun2, c->stream.get()))
            return fail(c, FTTE_ERR_NO_DEVICE, who + "kernel launch failed");
        if ((rc = download(c, src_abun2, K.src_abun2, sizeof(double) * ns))) return rc;
    }
    return FTTE_OK;
}

int ftte_star_populations(int nmetal, const double *metallicity, int64_t nsrc, const double *abun2, int32_t *iMetal, double *coefMetal,
                          int32_t *src_slot, int64_t *npop, int64_t *pop_first)
{
    if (nmetal < 2 || !metallicity || nsrc < 0 || (nsrc > 0 && !abun2))
        return fail(nullptr, FTTE_ERR_ARG, "ftte_star_populations: bad argument");
    const size_t ns = (size_t)nsrc;
    std::vector<int32_t> im, slot;
    std::vector<double> cm;
    if (!iMetal) { im.resize(ns); iMetal = im.data(); }
    if (!coefMetal) { cm.resize(ns); coefMetal = cm.data(); }
    if (!src_slot) { slot.resize(ns); src_slot = slot.data(); }
    for (size_t s = 0; s < ns; ++s) catalogue_metal_bracket(abun2[s], nmetal, metallicity, &iMetal[s], &coefMetal[s]);
    const int64_t slots = catalogue_slots(nsrc, iMetal, coefMetal, src_slot, pop_first);
    if (npop) *npop = slots;
    return FTTE_OK;
}

int ftte_cell_position(ftte_ctx *c, int64_t cell, int *level, int32_t *position)
{
    int rc = check_ready(c, false);
    if (rc) return rc;
    if (cell < 0 || cell >= c->ncell) return fail(c, FTTE_ERR_ARG, "ftte_cell_position: cell outside the cell array");
    const AmrTree &T = c->tree;
    int32_t at = T.refined() ? c->catalogue.leaf_nodes(T)[(size_t)cell] : (int32_t)cell;
    const int depth = T.refined() ? (int)T.level[(size_t)at] : 0;
    if (level) *level = depth;
    if (!position) return FTTE_OK;
    for (int l = depth; l >= 1; --l) {
        const int32_t up = T.parent[(size_t)at];
        const int child = at - T.child0[(size_t)up];
        position[3 * l] = (child >> 2) + 1;
        position[3 * l + 1] = ((child >> 1) & 1) + 1;
        position[3 * l + 2] = (child & 1) + 1;
        at = up;
    }
    const int n = c->n;
    position[0] = at / (n * n) + 1;
    position[1] = (at / n) % n + 1;
    position[2] = at % n + 1;
    return FTTE_OK;
}

} // extern "C"
