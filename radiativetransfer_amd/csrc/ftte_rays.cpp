// ftte_rays.cpp -- the oblique-ray entry points of include/ftte.h: absorption spectra along rays of any origin and direction
// through the refined grid, and the rays' segment lists (kernels: ftte_rays.hip; the walk's statement: ftte_ray_math.h; the line's:
// ftte_spectra_math.h; the context-free batch rule: ftte_rays.h).  The kernels read GasState::field(f), ChemState::tgas, the three
// components of the velocity field and the tracer's NodeRec tree where they lie.  Working memory is ftte_ctx::spectra's.
#include "ftte_rays.h"

#include "ftte_context.h"

using namespace ftte;

namespace {

struct RayCall {
    const char *who;
    int64_t nray;
    const double *origin, *dir, *tmax; // host arrays
    bool periodic;                     // the rays go on through the box's opposite face up to tmax
    // the spectra
    bool spectra;
    int nvel;
    double v0, dv, hubble, period;
    const double *line;
    const double *value;
    bool on_device; // value, tau and summary are device pointers
    double *tau, *summary;
    // the segment list
    int64_t *offset, capacity, *leaf;
    double *t_in, *t_out;
};

bool finite(double v) { return std::isfinite(v); }

int run_rays(ftte_ctx *c, const RayCall &M)
{
    int rc = check_ready(c, false);
    if (rc) return rc;
    const std::string who = std::string(M.who) + ": ";
    RayRec R;
    std::memset(&R, 0, sizeof R);
    if (M.nray < 1 || !M.origin || !M.dir) return fail(c, FTTE_ERR_ARG, who + "nray must be at least 1; origin and dir must be given");
    if (M.nray > ((int64_t)1 << 30)) return fail(c, FTTE_ERR_UNSUPPORTED, who + "more than 2^30 rays");
    if (M.spectra) {
        if (!M.line || (!M.tau && !M.summary)) return fail(c, FTTE_ERR_ARG, who + "bad argument");
        if (M.nvel < 1) return fail(c, FTTE_ERR_ARG, who + "nvel must be at least 1");
        if (!(M.dv > 0.0) || !finite(M.dv) || !finite(M.v0) || !finite(M.hubble)) return fail(c, FTTE_ERR_ARG, who + "dv must be positive; v0, dv and hubble finite");
        if (!(M.period >= 0.0) || !finite(M.period)) return fail(c, FTTE_ERR_ARG, who + "period must not be negative");
        const double sigma = M.line[0], damping = M.line[1], mass = M.line[2], bturb = M.line[3];
        if (!(mass > 0.0) || !finite(mass)) return fail(c, FTTE_ERR_ARG, who + "the absorber's mass must be positive");
        if (!(damping >= 0.0) || !finite(damping) || !(bturb >= 0.0) || !finite(bturb)) return fail(c, FTTE_ERR_ARG, who + "damping and b_turb must not be negative");
        if (!finite(sigma)) return fail(c, FTTE_ERR_ARG, who + "sigma_line must be finite");
        R.par.v0 = M.v0; R.par.dv = M.dv; R.par.hubble = M.hubble;
        R.par.period = M.period; R.par.inv_period = M.period > 0.0 ? 1.0 / M.period : 0.0;
        R.par.sigma = sigma; R.par.damping = damping; R.par.mass = mass; R.par.bturb = bturb;
    } else {
        if (!M.offset || M.capacity < 0) return fail(c, FTTE_ERR_ARG, who + "offset must be given and capacity must not be negative");
        if (M.capacity > 0 && (!M.leaf || !M.t_in || !M.t_out)) return fail(c, FTTE_ERR_ARG, who + "leaf, t_in and t_out must be given with a capacity");
    }
    for (int64_t r = 0; r < M.nray; ++r)
        if (!ray_arguments_ok(M.origin + 3 * r, M.dir + 3 * r, M.tmax ? M.tmax + r : nullptr))
            return fail(c, FTTE_ERR_ARG, who + "ray " + std::to_string(r) + ": origin, direction and tmax must be finite and | |dir|^2 - 1 | <= 1e-9");
    double longest = 0.0;
    if (M.periodic) {
        if (!M.tmax) return fail(c, FTTE_ERR_ARG, who + "ray 0: a periodic ray needs its tmax");
        for (int64_t r = 0; r < M.nray; ++r) {
            const int refusal = ray_periodic_refusal(M.origin + 3 * r, M.tmax + r, c->n);
            if (refusal == 1) return fail(c, FTTE_ERR_ARG, who + "ray " + std::to_string(r) + ": the tmax of a periodic ray must be greater than 0");
            if (refusal) return fail(c, FTTE_ERR_UNSUPPORTED, who + "ray " + std::to_string(r) + ": origin more than 2^20 boxes away");
            if (M.tmax[r] > longest) longest = M.tmax[r];
        }
    }
    if (M.spectra) {
        if (!c->gas.ready(c->ncell)) return fail(c, FTTE_ERR_STATE, who + "no medium: call ftte_set_medium first");
        if (!c->chem.temperature_set) return fail(c, FTTE_ERR_STATE, who + "no temperature (ftte_set_temperature)");
    }
    R.max_steps = M.periodic ? ray_step_bound_periodic(c->n, c->tree.max_level, longest) : ray_step_bound(c->n, c->tree.max_level);
    if (R.max_steps < 1) {
        if (c->tree.max_level > FTTE_RAY_MAX_LEVEL || !M.periodic) return fail(c, FTTE_ERR_UNSUPPORTED, who + "tree deeper than 40 levels");
        if (longest / (double)c->n > FTTE_RAY_MAX_BOXES) return fail(c, FTTE_ERR_UNSUPPORTED, who + "a periodic ray longer than 2^20 boxes");
        return fail(c, FTTE_ERR_UNSUPPORTED, who + "the step bound of the longest periodic ray is beyond 2^62");
    }
    R.periodic = M.periodic ? 1 : 0;

    FTTE_HIP(c, hipSetDevice(c->device));
    if ((rc = wait_sweep(c))) return rc;
    SpectraState &S = c->spectra;
    FTTE_HIP(c, c->dtree.ensure(c->stream, c->tree));
    const size_t nray = (size_t)M.nray;
    FTTE_HIP(c, S.ray_origin.reserve(3 * nray));
    FTTE_HIP(c, S.ray_dir.reserve(3 * nray));
    if ((rc = upload(c, S.ray_origin, M.origin, sizeof(double) * 3 * nray))) return rc;
    if ((rc = upload(c, S.ray_dir, M.dir, sizeof(double) * 3 * nray))) return rc;
    if (M.tmax) {
        FTTE_HIP(c, S.ray_tmax.reserve(nray));
        if ((rc = upload(c, S.ray_tmax, M.tmax, sizeof(double) * nray))) return rc;
    }
    const double *value = nullptr;
    if (M.spectra) {
        value = M.value;
        if (value && !M.on_device) {
            FTTE_HIP(c, S.value.reserve((size_t)c->ncell));
            if ((rc = upload(c, S.value, value, sizeof(double) * (size_t)c->ncell))) return rc;
            value = S.value;
        }
        if (!value) value = c->gas.field(GasState::kHI);
    }
    FTTE_HIP(c, S.nseg.reserve(nray));
    FTTE_HIP(c, S.column.reserve(nray));
    FTTE_HIP(c, S.flags.reserve(3));
    FTTE_HIP(c, S.ray_offset.reserve(nray + 1));
    FTTE_HIP(c, hipMemsetAsync(S.flags, 0, 3 * sizeof(int32_t), c->stream));

    R.node = c->dtree.nodes();
    R.origin = S.ray_origin; R.dir = S.ray_dir; R.tmax = M.tmax ? S.ray_tmax.get() : nullptr;
    R.nray = M.nray;
    R.n = c->n;
    R.value = value;
    R.tgas = M.spectra ? c->chem.tgas.get() : nullptr;
    if (M.spectra && S.velocity_set) { R.velx = S.vel[0]; R.vely = S.vel[1]; R.velz = S.vel[2]; }
    R.cell_cm = c->box / (double)c->n;
    R.K = kMath;
    R.nseg = S.nseg; R.column = S.column; R.flags = S.flags;
    R.nvel = M.nvel;

    // count mode: every ray's segments, and every leaf on a ray has a line width and no walk passed its bound, or nothing of the
    // caller's is written.  The offsets are the host's prefix sum over the counts (4 bytes per ray down, 8 up).
    int32_t flags[3] = {0, 0, 0};
    std::vector<int32_t> count(nray);
    hipError_t e = hipSuccess, e2 = hipSuccess;
    int lrc = launch_ray_walk(R, false, c->stream.get());
    if (!lrc) {
        e = hipMemcpyAsync(flags, S.flags, sizeof flags, hipMemcpyDeviceToHost, c->stream);
        e2 = hipMemcpyAsync(count.data(), S.nseg, sizeof(int32_t) * nray, hipMemcpyDeviceToHost, c->stream);
    }
    hipError_t es = hipStreamSynchronize(c->stream);
    if (lrc) return fail(c, lrc == -1 ? FTTE_ERR_ARG : FTTE_ERR_NO_DEVICE, who + "kernel launch failed");
    if (e != hipSuccess || e2 != hipSuccess || es != hipSuccess) return fail(c, FTTE_ERR_NO_DEVICE, who + hipGetErrorString(e != hipSuccess ? e : e2 != hipSuccess ? e2 : es));
    if (flags[2]) return fail(c, FTTE_ERR_INTERNAL, who + "a ray's walk passed its step bound");
    if (flags[0]) return fail(c, FTTE_ERR_ARG, who + "2 k_B T / mass + b_turb^2 of a leaf on a ray is not positive and finite");
    std::vector<int64_t> offset(nray + 1);
    offset[0] = 0;
    for (size_t r = 0; r < nray; ++r) offset[r + 1] = offset[r] + count[r];
    const int64_t total = offset[nray];
    if (!M.spectra) {
        if (M.capacity > 0 && M.capacity < total) return fail(c, FTTE_ERR_ARG, who + "capacity below the number of segments (" + std::to_string(total) + ")");
        std::memcpy(M.offset, offset.data(), sizeof(int64_t) * (nray + 1));
        if (M.capacity == 0 || total == 0) return FTTE_OK;
    }
    FTTE_HIP(c, hipMemcpyAsync(S.ray_offset, offset.data(), sizeof(int64_t) * (nray + 1), hipMemcpyHostToDevice, c->stream));
    FTTE_HIP(c, hipStreamSynchronize(c->stream)); // (`offset` is pageable)
    R.offset = S.ray_offset;

    const bool stage_tau = M.spectra && !(M.on_device && M.tau), stage_summary = M.spectra && M.summary && !M.on_device;
    const size_t per_segment = M.spectra ? sizeof(ftte_spectra_seg) : kRaySegmentListBytes;
    for (int64_t ray0 = 0; ray0 < M.nray;) {
        const int64_t nr = ray_batch_rays(offset.data(), M.nray, ray0, M.nvel, stage_tau, per_segment);
        const size_t segs = (size_t)(offset[(size_t)(ray0 + nr)] - offset[(size_t)ray0]);
        R.ray0 = ray0;
        R.nrays = (int32_t)nr;
        if (M.spectra) {
            FTTE_HIP(c, S.ray_rec.reserve(segs));
            if (stage_tau) FTTE_HIP(c, S.tau.reserve((size_t)nr * (size_t)M.nvel));
            if (stage_summary) FTTE_HIP(c, S.summary.reserve((size_t)nr * 3));
            R.rec = S.ray_rec;
            R.tau = stage_tau ? S.tau.get() : M.tau + ray0 * M.nvel;
            R.summary = !M.summary ? nullptr : stage_summary ? S.summary.get() : M.summary + ray0 * 3;
            if (segs && (lrc = launch_ray_walk(R, true, c->stream.get()))) return fail(c, lrc == -1 ? FTTE_ERR_ARG : FTTE_ERR_NO_DEVICE, who + "kernel launch failed");
            if ((lrc = launch_ray_spectra(R, c->stream.get()))) return fail(c, lrc == -1 ? FTTE_ERR_ARG : FTTE_ERR_NO_DEVICE, who + "kernel launch failed");
            if (!M.on_device) {
                if (M.tau && (rc = download(c, M.tau + ray0 * M.nvel, S.tau, sizeof(double) * (size_t)nr * (size_t)M.nvel))) return rc;
                if (M.summary && (rc = download(c, M.summary + ray0 * 3, S.summary, sizeof(double) * (size_t)nr * 3))) return rc;
            }
        } else if (segs) {
            FTTE_HIP(c, S.ray_leaf.reserve(segs));
            FTTE_HIP(c, S.ray_tin.reserve(segs));
            FTTE_HIP(c, S.ray_tout.reserve(segs));
            R.leaf = S.ray_leaf; R.t_in = S.ray_tin; R.t_out = S.ray_tout;
            if ((lrc = launch_ray_walk(R, true, c->stream.get()))) return fail(c, lrc == -1 ? FTTE_ERR_ARG : FTTE_ERR_NO_DEVICE, who + "kernel launch failed");
            const size_t at = (size_t)offset[(size_t)ray0];
            if ((rc = download(c, M.leaf + at, S.ray_leaf, sizeof(int64_t) * segs))) return rc;
            if ((rc = download(c, M.t_in + at, S.ray_tin, sizeof(double) * segs))) return rc;
            if ((rc = download(c, M.t_out + at, S.ray_tout, sizeof(double) * segs))) return rc;
        }
        ray0 += nr;
    }
    FTTE_HIP(c, hipStreamSynchronize(c->stream));
    return FTTE_OK;
}

RayCall spectra_call(const char *who, bool periodic, int64_t nray, const double *origin, const double *dir, const double *tmax, int nvel, double v0, double dv,
                     double hubble, double period, const double *line, const double *value, bool on_device, double *tau, double *summary)
{
    RayCall M;
    std::memset(&M, 0, sizeof M);
    M.who = who; M.nray = nray; M.origin = origin; M.dir = dir; M.tmax = tmax; M.periodic = periodic;
    M.spectra = true;
    M.nvel = nvel; M.v0 = v0; M.dv = dv; M.hubble = hubble; M.period = period; M.line = line; M.value = value;
    M.on_device = on_device; M.tau = tau; M.summary = summary;
    return M;
}

int segments_call(ftte_ctx *c, const char *who, bool periodic, int64_t nray, const double *origin, const double *dir, const double *tmax, int64_t *offset,
                  int64_t capacity, int64_t *leaf, double *t_in, double *t_out)
{
    RayCall M;
    std::memset(&M, 0, sizeof M);
    M.who = who; M.nray = nray; M.origin = origin; M.dir = dir; M.tmax = tmax; M.periodic = periodic;
    M.offset = offset; M.capacity = capacity; M.leaf = leaf; M.t_in = t_in; M.t_out = t_out;
    return run_rays(c, M);
}

} // namespace

extern "C" {

int ftte_ray_spectra(ftte_ctx *c, int64_t nray, const double *origin, const double *dir, const double *tmax, int nvel, double v0, double dv, double hubble,
                     double period, const double *line, const double *value, double *tau, double *summary)
{
    return run_rays(c, spectra_call("ftte_ray_spectra", false, nray, origin, dir, tmax, nvel, v0, dv, hubble, period, line, value, false, tau, summary));
}

int ftte_ray_spectra_periodic(ftte_ctx *c, int64_t nray, const double *origin, const double *dir, const double *tmax, int nvel, double v0, double dv, double hubble,
                              double period, const double *line, const double *value, double *tau, double *summary)
{
    return run_rays(c, spectra_call("ftte_ray_spectra_periodic", true, nray, origin, dir, tmax, nvel, v0, dv, hubble, period, line, value, false, tau, summary));
}

int ftte_ray_spectra_device(ftte_ctx *c, int64_t nray, const double *origin, const double *dir, const double *tmax, int nvel, double v0, double dv,
                            double hubble, double period, const double *line, const double *value_dev, double *tau_dev, double *summary_dev)
{
    return run_rays(c, spectra_call("ftte_ray_spectra_device", false, nray, origin, dir, tmax, nvel, v0, dv, hubble, period, line, value_dev, true, tau_dev, summary_dev));
}

int ftte_ray_spectra_periodic_device(ftte_ctx *c, int64_t nray, const double *origin, const double *dir, const double *tmax, int nvel, double v0, double dv,
                                     double hubble, double period, const double *line, const double *value_dev, double *tau_dev, double *summary_dev)
{
    return run_rays(c, spectra_call("ftte_ray_spectra_periodic_device", true, nray, origin, dir, tmax, nvel, v0, dv, hubble, period, line, value_dev, true, tau_dev,
                                    summary_dev));
}

int ftte_ray_segments(ftte_ctx *c, int64_t nray, const double *origin, const double *dir, const double *tmax, int64_t *offset, int64_t capacity, int64_t *leaf,
                      double *t_in, double *t_out)
{
    return segments_call(c, "ftte_ray_segments", false, nray, origin, dir, tmax, offset, capacity, leaf, t_in, t_out);
}

int ftte_ray_segments_periodic(ftte_ctx *c, int64_t nray, const double *origin, const double *dir, const double *tmax, int64_t *offset, int64_t capacity,
                               int64_t *leaf, double *t_in, double *t_out)
{
    return segments_call(c, "ftte_ray_segments_periodic", true, nray, origin, dir, tmax, offset, capacity, leaf, t_in, t_out);
}

} // extern "C"
