// ftte_point.cpp -- host side of the point-source path.  See ftte_point.h.
#include "ftte_point.h"

#include <algorithm>
#include <cstring>

#include "ftte_chem_math.h"
#include "ftte_point_rec.h"

namespace ftte {

namespace {

int hip_fail(std::string *err, const char *what, hipError_t e)
{
    *err = std::string(what) + ": " + hipGetErrorString(e);
    return FTTE_ERR_NO_DEVICE;
}

#define POINT_HIP(call)                                                                                            \
    do {                                                                                                           \
        hipError_t e_ = (call);                                                                                    \
        if (e_ != hipSuccess) return hip_fail(err, #call, e_);                                                     \
    } while (0)

} // namespace

// ---- the rate tables ------------------------------------------------------------------------------------------------

int RateTables::missing(bool slots, std::string *err) const
{
    if (by_slot(slots).count) return 0;
    *err = slots ? "no population slots: call ftte_stellar_beta_tables or ftte_set_population_tables first"
                 : "no rate tables: call ftte_stellar_beta_table or ftte_set_rate_tables first";
    return FTTE_ERR_STATE;
}

// Room for npop slots.  What is missing is compared with the free device memory (plus what the buffers to be replaced give back)
// before anything is released, so that this refusal leaves the slots held as they were.  From the moment a slot buffer is
// replaced no slot is held, until the caller has filled the new ones: also where the allocation itself or a later step fails.
int RateTables::reserve_slots(int npop, bool with_bins, std::string *err)
{
    const size_t want = (size_t)npop * kSetDoubles, want_bins = with_bins ? (size_t)npop * kFrequencies : 0;
    size_t need = 0, back = 0;
    for (const DeviceBuffer<double> *b : {&slots_.tables, &slots_.logtab})
        if (b->capacity() < want) { need += want * sizeof(double); back += b->capacity() * sizeof(double); }
    if (bins_.capacity() < want_bins) { need += want_bins * sizeof(FreqBin); back += bins_.capacity() * sizeof(FreqBin); }
    if (need) {
        size_t free_bytes = 0, total_bytes = 0;
        POINT_HIP(hipMemGetInfo(&free_bytes, &total_bytes));
        if (need > free_bytes + back) {
            *err = "population slots: " + std::to_string(npop) + " slots need " + std::to_string(need) + " bytes of device memory, " +
                   std::to_string(free_bytes + back) + " are free";
            return FTTE_ERR_MEMORY;
        }
    }
    if (slots_.reserve(npop) != hipSuccess || bins_.reserve(want_bins) != hipSuccess) {
        (void)hipGetLastError();
        slots_ = TableSets();
        *err = "population slots: " + std::to_string(need) + " bytes of device memory could not be allocated";
        return FTTE_ERR_MEMORY;
    }
    return 0;
}

// The bins of n populations are on the host: n sets of S from them, one launch for all.  Returns when `bins` may go.
int RateTables::fill_from_bins(TableSets &S, hipStream_t stream, const std::vector<FreqBin> &bins, int n, std::string *err)
{
    S.count = 0;
    POINT_HIP(hipMemcpyAsync(bins_, bins.data(), sizeof(FreqBin) * bins.size(), hipMemcpyHostToDevice, stream));
    if (launch_rate_table(bins_, (int)bins.size() / n, n, S.tables, S.logtab, stream)) { *err = "rate table kernel failed to launch"; return FTTE_ERR_NO_DEVICE; }
    POINT_HIP(hipStreamSynchronize(stream));
    S.count = n;
    return 0;
}

// n sets of S from the host, and their logarithms
int RateTables::fill_from_host(TableSets &S, hipStream_t stream, const double *tables, int n, std::string *err)
{
    S.count = 0;
    POINT_HIP(hipMemcpyAsync(S.tables, tables, sizeof(double) * kSetDoubles * n, hipMemcpyHostToDevice, stream));
    if (launch_log_table(S.tables, n, S.logtab, stream)) { *err = "table kernel failed to launch"; return FTTE_ERR_NO_DEVICE; }
    POINT_HIP(hipStreamSynchronize(stream));
    S.count = n;
    return 0;
}

int RateTables::set_sigma(hipStream_t stream, const double *sigma, std::string *err)
{
    // the tracer multiplies the threshold depths by sigma(E) / sigma(threshold), :3216-3219
    double ratio[4 * kOutputEnergies];
    const double thr[4] = {FTTE_SIGMA_HI, FTTE_SIGMA_HEII, FTTE_SIGMA_HEI, kSigmaDustThreshold};
    for (int q = 0; q < 4; ++q)
        for (int ie = 0; ie < kOutputEnergies; ++ie) ratio[q * kOutputEnergies + ie] = sigma[q * kOutputEnergies + ie] / thr[q];
    POINT_HIP(sigma_ratio_.reserve((size_t)4 * kOutputEnergies));
    POINT_HIP(hipMemcpyAsync(sigma_ratio_, ratio, sizeof ratio, hipMemcpyHostToDevice, stream));
    POINT_HIP(hipStreamSynchronize(stream));
    sigma_ready_ = true;
    return 0;
}

int RateTables::set_current(hipStream_t stream, const double *tables, std::string *err)
{
    sigma_ready_ = false;
    POINT_HIP(current_.reserve(1));
    return fill_from_host(current_, stream, tables, 1, err);
}

int RateTables::current_from_bins(hipStream_t stream, const std::vector<FreqBin> &bins, const double *sigma, std::string *err)
{
    int rc;
    if ((rc = set_sigma(stream, sigma, err))) return rc;
    POINT_HIP(current_.reserve(1));
    POINT_HIP(bins_.reserve((size_t)kFrequencies));
    return fill_from_bins(current_, stream, bins, 1, err);
}

int RateTables::slots_from_bins(hipStream_t stream, const std::vector<FreqBin> &bins, int npop, const double *sigma, std::string *err)
{
    int rc;
    if ((rc = reserve_slots(npop, true, err))) return rc;
    if ((rc = set_sigma(stream, sigma, err))) return rc;
    return fill_from_bins(slots_, stream, bins, npop, err);
}

int RateTables::set_slots(hipStream_t stream, int npop, const double *tables, std::string *err)
{
    int rc;
    if ((rc = reserve_slots(npop, false, err))) return rc;
    return fill_from_host(slots_, stream, tables, npop, err);
}

int RateTables::get(hipStream_t stream, bool slots, int k, double *tables, std::string *err) const
{
    POINT_HIP(hipMemcpyAsync(tables, by_slot(slots).tables + (size_t)k * kSetDoubles, sizeof(double) * kSetDoubles, hipMemcpyDeviceToHost, stream));
    POINT_HIP(hipStreamSynchronize(stream));
    return 0;
}

int point_stellar_beta_table(RateTables &R, hipStream_t stream, const double *a_smc, int nwave, const double *wavelength,
                             int nspectrum, int nmetal, const double *spec, int iSpectrum, double cS, int iMetal, double cM,
                             double *total_integral, std::string *err)
{
    static thread_local FrequencyGrid G;
    frequency_grid(a_smc, G);
    std::vector<FreqBin> bins(kFrequencies - 1);
    const double total = population_bins(G, spec, nmetal, nspectrum, nwave, wavelength, iSpectrum, cS, iMetal, cM, bins.data());
    if (total_integral) *total_integral = total;
    double sigma[4 * kOutputEnergies];
    output_sigma(a_smc, sigma);
    return R.current_from_bins(stream, bins, sigma, err);
}

int point_stellar_beta_tables(RateTables &R, hipStream_t stream, const double *a_smc, int nwave, const double *wavelength,
                              int nspectrum, int nmetal, const double *spec, int npop, const int *iSpectrum, const double *cS,
                              const int *iMetal, const double *cM, double *total_integral, std::string *err)
{
    static thread_local FrequencyGrid G;
    frequency_grid(a_smc, G);
    const int nbins = kFrequencies - 1;
    std::vector<FreqBin> bins((size_t)npop * nbins);
    for (int p = 0; p < npop; ++p) {
        const double total = population_bins(G, spec, nmetal, nspectrum, nwave, wavelength, iSpectrum[p], cS[p], iMetal[p], cM[p],
                                             bins.data() + (size_t)p * nbins);
        if (total_integral) total_integral[p] = total;
    }
    double sigma[4 * kOutputEnergies];
    output_sigma(a_smc, sigma);
    return R.slots_from_bins(stream, bins, npop, sigma, err);
}

int point_lookup(PointState &P, hipStream_t stream, int dust, int nsample, const double *tau, double *rates, std::string *err)
{
    if (const int rc = P.tables.missing(false, err)) return rc;
    POINT_HIP(P.sample_in.reserve((size_t)4 * nsample));
    POINT_HIP(P.sample_out.reserve((size_t)6 * nsample));
    POINT_HIP(hipMemcpyAsync(P.sample_in, tau, sizeof(double) * 4 * nsample, hipMemcpyHostToDevice, stream));
    if (launch_rate_lookup(P.tables.by_slot(false).logtab, dust, nsample, P.sample_in, P.sample_out, stream)) { *err = "look-up kernel failed to launch"; return FTTE_ERR_NO_DEVICE; }
    POINT_HIP(hipMemcpyAsync(rates, P.sample_out, sizeof(double) * 6 * nsample, hipMemcpyDeviceToHost, stream));
    POINT_HIP(hipStreamSynchronize(stream));
    return 0;
}

int point_set_medium(GasState &G, hipStream_t stream, int64_t ncell, const double *const field[5], bool on_device, int dust,
                     std::string *err)
{
    POINT_HIP(G.reserve(ncell));
    for (int f = 0; f < GasState::kFields; ++f) {
        if (field[f])
            POINT_HIP(hipMemcpyAsync(G.field(f), field[f], sizeof(double) * ncell, on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, stream));
        else
            POINT_HIP(hipMemsetAsync(G.field(f), 0, sizeof(double) * ncell, stream)); // rho, abun2 are only read with dust
    }
    POINT_HIP(hipStreamSynchronize(stream));
    G.filled(ncell, dust, field[GasState::kRho] != nullptr, field[GasState::kAbun2] != nullptr);
    return 0;
}

// ---- the accumulated rates ------------------------------------------------------------------------------------------

int PointRates::zero(hipStream_t stream, int64_t ncell, std::string *err)
{
    if (cells_ != ncell) drop();
    POINT_HIP(rates_.reserve((size_t)kCellRec * ncell));
    cells_ = ncell;
    POINT_HIP(hipMemsetAsync(rates_, 0, sizeof(double) * kCellRec * ncell, stream));
    return 0;
}

int PointRates::planes(hipStream_t stream, double **planes, std::string *err)
{
    POINT_HIP(planes_.reserve((size_t)6 * cells_));
    if (launch_repack_rates(planes_, rates_, (long)cells_, false, stream)) { *err = "layout kernel failed to launch"; return FTTE_ERR_NO_DEVICE; }
    *planes = planes_;
    return 0;
}

int PointRates::set(hipStream_t stream, int64_t ncell, const double *planes_host, std::string *err)
{
    int rc;
    if ((rc = zero(stream, ncell, err))) return rc;
    POINT_HIP(planes_.reserve((size_t)6 * ncell));
    POINT_HIP(hipMemcpyAsync(planes_, planes_host, sizeof(double) * 6 * ncell, hipMemcpyHostToDevice, stream));
    if (launch_repack_rates(planes_, rates_, (long)ncell, true, stream)) { *err = "layout kernel failed to launch"; return FTTE_ERR_NO_DEVICE; }
    POINT_HIP(hipStreamSynchronize(stream));
    return 0;
}

// ---- the tracer: point_trace and its steps ---------------------------------------------------------------------------

int check_sources(const DeviceTree &D, int64_t ncell, int nsrc, const int64_t *cell, const int32_t *slot, int nslots, int32_t *node,
                  std::string *err)
{
    for (int s = 0; s < nsrc; ++s) {
        if (cell[s] < 0 || cell[s] >= ncell) { *err = "ftte_point_sources: source cell outside the cell array"; return FTTE_ERR_ARG; }
        node[s] = D.node_of(cell[s]);
    }
    if (slot)
        for (int s = 0; s < nsrc; ++s)
            if (slot[s] < 0 || slot[s] >= nslots) {
                *err = "ftte_point_sources_populations: star " + std::to_string(s) + " names slot " + std::to_string(slot[s]) +
                       ", outside 0.." + std::to_string(nslots - 1);
                return FTTE_ERR_ARG;
            }
    return 0;
}

const char *trace_error_text(int code)
{
    static const char *what[] = {"", "continuation cell outside the base grid", "error in checkPoint (start)",
                                 "error in checkPoint", "ray did not terminate", "split queue overflow"};
    return what[code >= 0 && code < 6 ? code : 3];
}

namespace {

// Tables and medium are there; the rates, the device tree, the packed medium, the pixel directions with rmax and the scratch are
// made where they are missing.  *batch: the stars of a batch.
int prepare_trace(PointState &P, DeviceTree &D, GasState &G, hipStream_t stream, const AmrTree &tree, int nsrc, bool by_slot, int *batch,
                  std::string *err)
{
    int rc;
    if ((rc = P.tables.missing(by_slot, err))) return rc;
    if (!G.ready(tree.ncell)) { *err = "no medium: call ftte_set_medium after ftte_set_grid"; return FTTE_ERR_STATE; }
    if (!P.rates.ready(tree.ncell))
        if ((rc = P.rates.zero(stream, tree.ncell, err))) return rc;
    POINT_HIP(D.ensure(stream, tree));
    POINT_HIP(G.reserve_packed(kCellRec));
    if (!G.packed_current()) {
        const double *const fields[5] = {G.field(0), G.field(1), G.field(2), G.field(3), G.field(4)};
        if (launch_pack_medium(fields, G.packed(), (long)tree.ncell, stream)) { *err = "layout kernel failed to launch"; return FTTE_ERR_NO_DEVICE; }
        G.packed_made();
    }
    if (!P.pixdir) {
        std::vector<double> dir((size_t)3 * kPixelCount);
        if (pixel_directions(dir.data())) { *err = "pix2ang_nest failed"; return FTTE_ERR_PIXEL; }
        POINT_HIP(P.pixdir.reserve(dir.size()));
        POINT_HIP(hipMemcpyAsync(P.pixdir, dir.data(), sizeof(double) * dir.size(), hipMemcpyHostToDevice, stream));
        POINT_HIP(hipStreamSynchronize(stream));
        rmax_table(P.rmax);
    }
    hipError_t why = hipSuccess;
    *batch = P.scratch.reserve(nsrc, by_slot, &why);
    if (!*batch) return hip_fail(err, "the tracer's scratch", why);
    return 0;
}

// What every launch of a trace reads, from the owners; the batch and the level fill in the rest
TraceRec trace_record(const PointState &P, const DeviceTree &D, const GasState &G, const AmrTree &tree, double box, bool by_slot)
{
    const TraceScratch &S = P.scratch;
    TraceRec T;
    std::memset(&T, 0, sizeof(T));
    T.sigma_ratio = P.tables.sigma();
    {
        static const float radii[kOutputRadii] = {0.1f, 0.3f, 1.f, 3.f, 10.f, 30.f, 100.f}; // outputRadius [kpc], equiSources.f90:10
        for (int ir = 0; ir < kOutputRadii; ++ir) T.out_radius_kpc[ir] = (double)radii[ir];
        T.kpc = kKpc;
    }
    T.node = D.nodes();
    T.n = tree.n; T.dust = G.dust(); T.ncell = tree.ncell; T.box = box;
    T.medium = G.packed();
    T.logtab = P.tables.by_slot(by_slot).logtab; T.pixdir = P.pixdir;
    T.slot_stride = (int64_t)6 * kTableSize;
    T.rmax[0] = 0.0;
    for (int L = 1; L <= kMaxPixelLevel; ++L) T.rmax[L] = P.rmax[L - 1];
    T.rates = P.rates.packed();
    T.src_node = S.src_node; T.src_ndot = S.src_ndot;
    T.out_count = S.counters + TraceScratch::kQueueLength; T.error = S.counters + TraceScratch::kError;
    T.steps = reinterpret_cast<unsigned long long *>(S.counters + TraceScratch::kSteps);
    T.out_capacity = (int32_t)std::min(S.queue[0].capacity(), S.queue[1].capacity());
    return T;
}

// Stars s0 .. s0 + ns - 1 of the call, level after level until no ray splits.  first: the call's first batch, which clears the
// error and the count of crossings.
int trace_batch(TraceScratch &S, TraceRec &T, hipStream_t stream, int s0, int ns, const int32_t *node, const double *ndot, bool by_slot,
                bool first, std::string *err)
{
    POINT_HIP(hipMemcpyAsync(S.src_node, node, sizeof(int32_t) * ns, hipMemcpyHostToDevice, stream));
    POINT_HIP(hipMemcpyAsync(S.src_ndot, ndot, sizeof(double) * ns, hipMemcpyHostToDevice, stream));
    // R.src counts from the batch's first star: everything indexed by it starts at s0
    T.escape = S.escape + (size_t)s0 * kEscapeRec;
    T.slot_of = by_slot ? S.src_slot + s0 : nullptr;
    T.highest_level = S.src_highest + s0;
    int32_t host_counters[4] = {0, 0, 0, 0}, nrec = 0;
    for (int L = 1; L <= kMaxPixelLevel; ++L) {
        T.pixel_level = L;
        T.nrays = rays_of_level(L, ns, nrec);
        if (T.nrays == 0) break;
        T.in = S.queue[L & 1];
        T.out = S.queue[(L + 1) & 1];
        // queue length back to zero, the error carried over
        host_counters[TraceScratch::kQueueLength] = 0;
        POINT_HIP(hipMemcpyAsync(S.counters, host_counters, sizeof(int32_t), hipMemcpyHostToDevice, stream));
        if (L == 1 && first) POINT_HIP(hipMemsetAsync(S.counters + TraceScratch::kError, 0, sizeof(int32_t) * (TraceScratch::kCounters - TraceScratch::kError), stream));
        if (launch_point_trace(T, stream)) { *err = "tracer kernel failed to launch"; return FTTE_ERR_NO_DEVICE; }
        POINT_HIP(hipMemcpyAsync(host_counters, S.counters, sizeof(int32_t) * 4, hipMemcpyDeviceToHost, stream));
        POINT_HIP(hipStreamSynchronize(stream));
        nrec = host_counters[TraceScratch::kQueueLength];
        if (host_counters[TraceScratch::kError]) {
            *err = std::string("ftte_point_sources: ") + trace_error_text(host_counters[TraceScratch::kError]);
            return FTTE_ERR_PATTERN;
        }
    }
    return 0;
}

// The crossings, the escape records and the highest levels of the call's stars to the host
int collect_trace(PointState &P, hipStream_t stream, int nsrc, const double *src_ndot, int *highest_pixel_level, int *highest_per_star,
                  std::string *err)
{
    const TraceScratch &S = P.scratch;
    unsigned long long steps = 0;
    POINT_HIP(hipMemcpyAsync(&steps, S.counters + TraceScratch::kSteps, sizeof steps, hipMemcpyDeviceToHost, stream));
    double *const records = P.escape.receive(nsrc, src_ndot);
    POINT_HIP(hipMemcpyAsync(records, S.escape, sizeof(double) * (size_t)nsrc * kEscapeRec, hipMemcpyDeviceToHost, stream));
    std::vector<int32_t> highest(nsrc);
    POINT_HIP(hipMemcpyAsync(highest.data(), S.src_highest, sizeof(int32_t) * (size_t)nsrc, hipMemcpyDeviceToHost, stream));
    POINT_HIP(hipStreamSynchronize(stream));
    P.escape.counted((long long)steps);
    if (highest_pixel_level) *highest_pixel_level = *std::max_element(highest.begin(), highest.end());
    if (highest_per_star) std::copy(highest.begin(), highest.end(), highest_per_star);
    return 0;
}

} // namespace

int point_trace(PointState &P, DeviceTree &D, GasState &G, hipStream_t stream, const AmrTree &tree, double box, int nsrc,
                const int64_t *src_cell, const double *src_ndot, const int32_t *src_slot, int *highest_pixel_level, int *highest_per_star,
                std::string *err)
{
    const bool by_slot = src_slot != nullptr;
    TraceScratch &S = P.scratch;
    int rc, batch = 0;
    if ((rc = prepare_trace(P, D, G, stream, tree, nsrc, by_slot, &batch, err))) return rc;
    std::vector<int32_t> node(nsrc);
    if ((rc = check_sources(D, tree.ncell, nsrc, src_cell, src_slot, P.tables.slot_count(), node.data(), err))) return rc;

    // all stars of the call at once; a batch reads from its first star on, as it does in the escape records
    if (by_slot) POINT_HIP(hipMemcpyAsync(S.src_slot, src_slot, sizeof(int32_t) * nsrc, hipMemcpyHostToDevice, stream));
    POINT_HIP(hipMemsetAsync(S.src_highest, 0, sizeof(int32_t) * (size_t)nsrc, stream)); // :1266
    POINT_HIP(hipMemsetAsync(S.escape, 0, sizeof(double) * (size_t)nsrc * kEscapeRec, stream)); // :1267-1270

    TraceRec T = trace_record(P, D, G, tree, box, by_slot);
    for (int s0 = 0; s0 < nsrc; s0 += batch) {
        const int ns = std::min(nsrc - s0, batch);
        if ((rc = trace_batch(S, T, stream, s0, ns, node.data() + s0, src_ndot + s0, by_slot, s0 == 0, err))) return rc;
    }
    return collect_trace(P, stream, nsrc, src_ndot, highest_pixel_level, highest_per_star, err);
}

} // namespace ftte
