// ftte_analysis.cpp -- the analysis entry points of include/ftte.h: slice and projected maps, the clumping factor, the gas and the
// stellar PDF of the device-resident medium (kernels: ftte_analysis.hip), and the context-free arithmetic of the map axes.  The
// kernels read GasState::field(f) and the tracer's NodeRec tree directly: there is no copy that could go stale.  What the analysis
// keeps on the device is ftte_ctx::analysis.
#include "ftte_analysis.h"

#include "ftte_chem_math.h"
#include "ftte_context.h"

using namespace ftte;

namespace ftte {

int map_axis(int n, int nmap, double centre, double zoom, bool quotient_first, int32_t *base, double *frac)
{
    if (n < 1 || nmap < 1 || !(zoom > 0.0) || !std::isfinite(zoom) || !std::isfinite(centre) || !base || !frac) return -1;
    // equiSources.f90:685-689: startPoint = max(centerPoint - 0.5/zoomFactor, 0.), endPoint = min(startPoint + 1./zoomFactor, 1.)
    const double lo = centre - 0.5 / zoom;
    const double start = lo > 0.0 ? lo : 0.0;
    const double hi = start + 1.0 / zoom;
    const double end = hi < 1.0 ? hi : 1.0;
    const float fn = (float)nmap;
    for (int i = 1; i <= nmap; ++i) {
        const float fi = (float)i - 0.5f;
        // :703 is (endPoint-startPoint)*(float(i)-0.5)/float(nxmap) + startPoint, left to right in double; readCellArray.f90:126 is
        // the single-precision quotient alone, which the whole box (start 0, end 1) leaves as it is
        const double x0 = quotient_first ? (end - start) * (double)(fi / fn) + start : (end - start) * (double)fi / (double)fn + start;
        const double scaled = x0 * (double)n;
        if (!(scaled >= 0.0) || !(scaled < (double)n)) return -1;
        const int i0 = (int)scaled + 1;                                // :704
        base[i - 1] = i0;
        frac[i - 1] = x0 * (double)(float)n - (double)(float)(i0 - 1); // :708
    }
    return 0;
}

int map_depth(int n, double centre, double zoom, int32_t *kstart, int32_t *kend)
{
    if (n < 1 || !(zoom > 0.0) || !std::isfinite(zoom) || !std::isfinite(centre) || !kstart || !kend) return -1;
    const double lo = centre - 0.5 / zoom, hi = centre + 0.5 / zoom; // :687-688
    const double zstart = lo > 0.0 ? lo : 0.0, zend = hi < 1.0 ? hi : 1.0;
    if (!(zstart * (double)n < (double)n) || !(zend * (double)n >= 0.0)) return -1;
    const int a = (int)(zstart * (double)n) + 1, b = (int)(zend * (double)n) + 1;
    *kstart = a > 1 ? a : 1; // :699
    *kend = b < n ? b : n;   // :700
    return 0;
}

bool map_zone(int izone, MapZone *Z, int *fast_is_j)
{
    ZoneMap m;
    if (!zone_map(izone, &m)) return false;
    for (int a = 0; a < 3; ++a) { Z->src[a] = m.src[a]; Z->mirror[a] = m.mirror[a] ? 1 : 0; }
    for (int i = 1; i <= 2; ++i)
        for (int j = 1; j <= 2; ++j)
            for (int k = 1; k <= 2; ++k) {
                int a, b, d;
                rotate_indices(i, j, k, 2, 2, 2, izone, &a, &b, &d);
                Z->child[4 * (i - 1) + 2 * (j - 1) + (k - 1)] = 4 * (a - 1) + 2 * (b - 1) + (d - 1);
            }
    // neighbouring lanes along the map axis that feeds the contiguous storage index; where the depth does, the one that feeds the next
    const int feeds = m.src[2] != 2 ? m.src[2] : m.src[1];
    *fast_is_j = feeds == 1;
    return true;
}

} // namespace ftte

namespace {

// what every analysis call asks first: a single-device context with a grid; the sweep that may still write what is read has ended
int analysis_ready(ftte_ctx *c)
{
    int rc = check_ready(c, false);
    if (rc) return rc;
    FTTE_HIP(c, hipSetDevice(c->device));
    return wait_sweep(c);
}

struct MapCall {
    const char *who;
    bool project;
    int izone, nxmap, nymap;
    const double *centre;
    double zoom, zslice;
    int mode;
    const double *value;
    bool value_on_device;
    float *map;
};

int make_map(ftte_ctx *c, const MapCall &M)
{
    int rc = check_ready(c, false);
    if (rc) return rc;
    const std::string who = std::string(M.who) + ": ";
    MapRec R;
    std::memset(&R, 0, sizeof R);
    if (!map_zone(M.izone, &R.zone, &R.fast_is_j)) return fail(c, FTTE_ERR_IZONE, who + "izone outside 1..24");
    if (M.nxmap < 1 || M.nymap < 1 || !M.centre || !M.map) return fail(c, FTTE_ERR_ARG, who + "bad argument");
    if (!(M.zoom > 0.0) || !std::isfinite(M.zoom)) return fail(c, FTTE_ERR_ARG, who + "zoom must be positive");
    if (!M.project && !(M.zslice >= 0.0 && M.zslice < 1.0)) return fail(c, FTTE_ERR_ARG, who + "zslice outside [0, 1)");
    if (M.project && M.mode != 0 && M.mode != 1) return fail(c, FTTE_ERR_ARG, who + "mode must be 0 (mass-weighted mean) or 1 (path integral)");
    const size_t npix = (size_t)M.nxmap * (size_t)M.nymap;
    if (npix > ((size_t)1 << 30)) return fail(c, FTTE_ERR_UNSUPPORTED, who + "more than 2^30 pixels");
    const GasState &G = c->gas;
    if (M.project ? !G.ready_with_density(c->ncell) : !G.ready(c->ncell))
        return fail(c, FTTE_ERR_STATE, who + (M.project ? "no medium with density (ftte_set_medium with rho)" : "no medium: call ftte_set_medium first"));

    std::vector<int32_t> base[2];
    std::vector<double> frac[2];
    const int extent[2] = {M.nxmap, M.nymap};
    for (int a = 0; a < 2; ++a) {
        base[a].resize((size_t)extent[a]);
        frac[a].resize((size_t)extent[a]);
        if (map_axis(c->n, extent[a], M.centre[a], M.zoom, !M.project, base[a].data(), frac[a].data()))
            return fail(c, FTTE_ERR_ARG, who + "the window leaves the box (centre, zoom)");
    }
    if (M.project) {
        if (map_depth(c->n, M.centre[2], M.zoom, &R.kstart, &R.kend)) return fail(c, FTTE_ERR_ARG, who + "the window leaves the box (centre, zoom)");
    } else {
        // readCellArray.f90:134-135
        R.kbase = (int)(M.zslice * (double)c->n) + 1;
        if (R.kbase < 1 || R.kbase > c->n) return fail(c, FTTE_ERR_ARG, who + "zslice outside [0, 1)");
        R.kfrac = M.zslice * (double)(float)c->n - (double)(float)(R.kbase - 1);
    }

    if ((rc = analysis_ready(c))) return rc;
    AnalysisState &A = c->analysis;
    FTTE_HIP(c, c->dtree.ensure(c->stream, c->tree));
    for (int a = 0; a < 2; ++a) {
        FTTE_HIP(c, A.base[a].reserve(base[a].size()));
        FTTE_HIP(c, A.frac[a].reserve(frac[a].size()));
        FTTE_HIP(c, hipMemcpyAsync(A.base[a], base[a].data(), sizeof(int32_t) * base[a].size(), hipMemcpyHostToDevice, c->stream));
        FTTE_HIP(c, hipMemcpyAsync(A.frac[a], frac[a].data(), sizeof(double) * frac[a].size(), hipMemcpyHostToDevice, c->stream));
    }
    FTTE_HIP(c, A.map.reserve(npix));
    const double *value = M.value;
    if (value && !M.value_on_device) {
        FTTE_HIP(c, A.value.reserve((size_t)c->ncell));
        FTTE_HIP(c, hipMemcpyAsync(A.value, value, sizeof(double) * (size_t)c->ncell, hipMemcpyHostToDevice, c->stream));
        value = A.value;
    }
    if (!value) value = G.field(M.project ? GasState::kAbun2 : GasState::kHI);

    R.node = c->dtree.nodes();
    R.value = value;
    R.rho = G.field(GasState::kRho);
    R.ibase = A.base[0]; R.jbase = A.base[1]; R.ifrac = A.frac[0]; R.jfrac = A.frac[1];
    R.map = A.map;
    R.n = c->n; R.nxmap = M.nxmap; R.nymap = M.nymap;
    R.mode = M.mode;
    R.cell_cm = c->box / (double)c->n; // physicalBoxSize/dfloat(nx), :715
    R.levels = c->tree.max_level + 1;
    if (R.levels > kMapLevels) return fail(c, FTTE_ERR_UNSUPPORTED, who + "tree deeper than 63 levels");
    double size = R.cell_cm;
    for (int d = 0; d < R.levels; ++d) {
        const double s = size / (double)1.e21f;
        R.cube[d] = s * s * s;
        size = size / 2.0;
    }
    hipError_t e = hipSuccess;
    const int lrc = M.project ? launch_project_map(R, c->stream.get()) : launch_slice_map(R, c->stream.get());
    if (!lrc) e = hipMemcpyAsync(M.map, A.map, sizeof(float) * npix, hipMemcpyDeviceToHost, c->stream);
    const hipError_t es = hipStreamSynchronize(c->stream); // (the tables are locals)
    if (lrc) return fail(c, lrc == -1 ? FTTE_ERR_ARG : FTTE_ERR_NO_DEVICE, who + "kernel launch failed");
    if (e != hipSuccess || es != hipSuccess) return fail(c, FTTE_ERR_NO_DEVICE, who + hipGetErrorString(e != hipSuccess ? e : es));
    return FTTE_OK;
}

// the censuses read rho and the leaves' levels
int census_ready(ftte_ctx *c, const std::string &who)
{
    int rc = check_ready(c, false);
    if (rc) return rc;
    if (!c->gas.ready_with_density(c->ncell)) return fail(c, FTTE_ERR_STATE, who + "no medium with density (ftte_set_medium with rho)");
    if ((rc = analysis_ready(c))) return rc;
    return ensure_level(c);
}

} // namespace

extern "C" {

int ftte_map_axis(int n, int nmap, double centre, double zoom, int32_t *base, double *frac)
{
    return map_axis(n, nmap, centre, zoom, false, base, frac) ? FTTE_ERR_ARG : FTTE_OK;
}

int ftte_slice_axis(int n, int nmap, double centre, double zoom, int32_t *base, double *frac)
{
    return map_axis(n, nmap, centre, zoom, true, base, frac) ? FTTE_ERR_ARG : FTTE_OK;
}

int ftte_map_depth(int n, double centre, double zoom, int32_t *kstart, int32_t *kend)
{
    return map_depth(n, centre, zoom, kstart, kend) ? FTTE_ERR_ARG : FTTE_OK;
}

int ftte_slice_map(ftte_ctx *c, int izone, int nxmap, int nymap, const double *centre, double zoom, double zslice, const double *value,
                   float *map)
{
    return make_map(c, MapCall{"ftte_slice_map", false, izone, nxmap, nymap, centre, zoom, zslice, 0, value, false, map});
}

int ftte_slice_map_device(ftte_ctx *c, int izone, int nxmap, int nymap, const double *centre, double zoom, double zslice,
                          const double *value_dev, float *map)
{
    return make_map(c, MapCall{"ftte_slice_map_device", false, izone, nxmap, nymap, centre, zoom, zslice, 0, value_dev, true, map});
}

int ftte_project_map(ftte_ctx *c, int izone, int nxmap, int nymap, const double *centre, double zoom, int mode, const double *value,
                     float *map)
{
    return make_map(c, MapCall{"ftte_project_map", true, izone, nxmap, nymap, centre, zoom, 0.0, mode, value, false, map});
}

int ftte_project_map_device(ftte_ctx *c, int izone, int nxmap, int nymap, const double *centre, double zoom, int mode,
                            const double *value_dev, float *map)
{
    return make_map(c, MapCall{"ftte_project_map_device", true, izone, nxmap, nymap, centre, zoom, 0.0, mode, value_dev, true, map});
}

int ftte_clumping(ftte_ctx *c, double *clumping, double *volume, double *mean_nh)
{
    const std::string who = "ftte_clumping: ";
    int rc = census_ready(c, who);
    if (rc) return rc;
    AnalysisState &A = c->analysis;
    FTTE_HIP(c, A.sums.reserve(kClumpParts));
    const ClumpRec R{c->chem.level, c->gas.field(GasState::kRho), c->ncell, A.sums};
    if (launch_clumping(R, c->stream.get())) return fail(c, FTTE_ERR_NO_DEVICE, who + "kernel launch failed");
    double out[3];
    FTTE_HIP(c, hipMemcpyAsync(out, A.sums + 3 * kClumpBlocks, sizeof out, hipMemcpyDeviceToHost, c->stream));
    FTTE_HIP(c, hipStreamSynchronize(c->stream));
    // equiSources.f90:672-674
    const double density = out[1] / out[0], density2 = out[2] / out[0];
    if (clumping) *clumping = density2 / (density * density);
    if (volume) *volume = out[0];
    if (mean_nh) *mean_nh = density;
    return FTTE_OK;
}

int ftte_gas_pdf(ftte_ctx *c, double *pdf, double *outside)
{
    const std::string who = "ftte_gas_pdf: ";
    int rc = check_ready(c, false);
    if (rc) return rc;
    if (!pdf || !outside) return fail(c, FTTE_ERR_ARG, who + "bad argument");
    if ((rc = census_ready(c, who))) return rc;
    AnalysisState &A = c->analysis;
    const int nlev = c->tree.max_level + 1;
    if (nlev > kPdfLevels) return fail(c, FTTE_ERR_UNSUPPORTED, who + "tree deeper than 63 levels");
    const size_t slots = (size_t)kPdfSlots * (size_t)nlev;
    FTTE_HIP(c, A.counts.reserve(slots));
    FTTE_HIP(c, hipMemsetAsync(A.counts, 0, sizeof(unsigned long long) * slots, c->stream));
    const PdfRec R{c->chem.level, c->gas.field(GasState::kRho), c->ncell, nlev, A.counts};
    if (launch_gas_pdf(R, c->stream.get())) return fail(c, FTTE_ERR_NO_DEVICE, who + "kernel launch failed");
    std::vector<unsigned long long> counts(slots);
    FTTE_HIP(c, hipMemcpyAsync(counts.data(), A.counts, sizeof(unsigned long long) * slots, hipMemcpyDeviceToHost, c->stream));
    FTTE_HIP(c, hipStreamSynchronize(c->stream));
    // a leaf of level L weighs 2.**(-3*L), a single-precision power (:4703): every term and every sum below is exact
    for (int b = 0; b < kPdfSlots; ++b) {
        double sum = 0.;
        for (int l = 0; l < nlev; ++l) sum += (double)counts[(size_t)b * nlev + l] * (double)std::ldexp(1.0f, -3 * l);
        if (b < kPdfBins) pdf[b] = sum;
        else *outside = sum;
    }
    return FTTE_OK;
}

int ftte_star_pdf(ftte_ctx *c, int nsrc, const int64_t *src_cell, int32_t *pdf, int32_t *outside, double *mean_host_HI)
{
    const std::string who = "ftte_star_pdf: ";
    int rc = check_ready(c, false);
    if (rc) return rc;
    if (nsrc < 0 || (nsrc > 0 && !src_cell) || !pdf || !outside) return fail(c, FTTE_ERR_ARG, who + "bad argument");
    for (int s = 0; s < nsrc; ++s)
        if (src_cell[s] < 0 || src_cell[s] >= c->ncell)
            return fail(c, FTTE_ERR_ARG, who + "host cell of source " + std::to_string(s) + " outside the cell array");
    if (!c->gas.ready_with_density(c->ncell)) return fail(c, FTTE_ERR_STATE, who + "no medium with density (ftte_set_medium with rho)");
    std::fill(pdf, pdf + kPdfBins, 0);
    *outside = 0;
    const size_t ns = (size_t)nsrc;
    std::vector<double> picked(2 * ns);
    if (nsrc > 0) {
        if ((rc = analysis_ready(c))) return rc;
        AnalysisState &A = c->analysis;
        FTTE_HIP(c, A.cells.reserve(ns));
        FTTE_HIP(c, A.picked.reserve(2 * ns));
        FTTE_HIP(c, hipMemcpyAsync(A.cells, src_cell, sizeof(int64_t) * ns, hipMemcpyHostToDevice, c->stream));
        if (launch_gather(c->gas.field(GasState::kRho), A.cells, nsrc, A.picked, c->stream.get()) ||
            launch_gather(c->gas.field(GasState::kHI), A.cells, nsrc, A.picked + ns, c->stream.get()))
            return fail(c, FTTE_ERR_NO_DEVICE, who + "kernel launch failed");
        FTTE_HIP(c, hipMemcpyAsync(picked.data(), A.picked, sizeof(double) * 2 * ns, hipMemcpyDeviceToHost, c->stream));
        FTTE_HIP(c, hipStreamSynchronize(c->stream));
    }
    // equiSources.f90:787-813 for the stars with weight > 0, in their order (host; libm's log10 as the reference's dlog10)
    const double pc = (double)3.08568025e18f;
    const double pc3 = pc * pc * pc;
    double mean = 0.;
    for (size_t s = 0; s < ns; ++s) {
        mean = mean + picked[ns + s];
        const int b = pdf_bin(std::log10(picked[s] / FTTE_MSUN * pc3));
        if (b < kPdfBins) pdf[b] += 1;
        else *outside += 1;
    }
    if (mean_host_HI) *mean_host_HI = mean / (double)(float)nsrc; // :813 (no star: 0/0, as there)
    return FTTE_OK;
}

} // extern "C"
