// ftte_spectra.cpp -- the spectra entry points of include/ftte.h: the velocity field on the device and the absorption spectra
// along the pixel columns of the projected map (kernels: ftte_spectra.hip; the statement: ftte_spectra_math.h; the
// context-free batch rule: ftte_spectra.h).  The kernels read GasState::field(f), ChemState::tgas, the velocity field and the tracer's NodeRec tree
// where they lie.  What the spectra keep on the device is ftte_ctx::spectra.
#include "ftte_spectra.h"

#include "ftte_context.h"

using namespace ftte;

namespace {

int set_velocity(ftte_ctx *c, const double *vx, const double *vy, const double *vz, bool on_device, const char *who_c)
{
    int rc = check_ready(c, false);
    if (rc) return rc;
    const std::string who = std::string(who_c) + ": ";
    FTTE_HIP(c, hipSetDevice(c->device));
    SpectraState &S = c->spectra;
    if (!vx && !vy && !vz) {
        FTTE_HIP(c, hipStreamSynchronize(c->stream));
        S.drop_velocity();
        return FTTE_OK;
    }
    if (!vx || !vy || !vz) return fail(c, FTTE_ERR_ARG, who + "three arrays, or three NULLs to drop the field");
    const double *src[3] = {vx, vy, vz};
    const size_t nc = (size_t)c->ncell;
    S.velocity_set = false;
    for (int a = 0; a < 3; ++a) {
        FTTE_HIP(c, S.vel[a].reserve(nc));
        if (on_device) FTTE_HIP(c, hipMemcpyAsync(S.vel[a], src[a], sizeof(double) * nc, hipMemcpyDeviceToDevice, c->stream));
        else if ((rc = upload(c, S.vel[a], src[a], sizeof(double) * nc))) return rc;
    }
    FTTE_HIP(c, hipStreamSynchronize(c->stream));
    S.velocity_set = true;
    return FTTE_OK;
}

struct SpectraCall {
    const char *who;
    int izone, nxmap, nymap;
    const double *centre;
    double zoom;
    int nvel;
    double v0, dv, hubble, period;
    const double *line;
    const double *value;
    bool on_device; // value, tau and summary are device pointers
    double *tau, *summary;
};

bool finite(double v) { return std::isfinite(v); }

int make_spectra(ftte_ctx *c, const SpectraCall &M)
{
    int rc = check_ready(c, false);
    if (rc) return rc;
    const std::string who = std::string(M.who) + ": ";
    SpectraRec R;
    std::memset(&R, 0, sizeof R);
    if (!map_zone(M.izone, &R.zone, &R.fast_is_j)) return fail(c, FTTE_ERR_IZONE, who + "izone outside 1..24");
    if (M.nxmap < 1 || M.nymap < 1 || !M.centre || !M.line || (!M.tau && !M.summary)) return fail(c, FTTE_ERR_ARG, who + "bad argument");
    if (!(M.zoom > 0.0) || !finite(M.zoom)) return fail(c, FTTE_ERR_ARG, who + "zoom must be positive");
    if (M.nvel < 1) return fail(c, FTTE_ERR_ARG, who + "nvel must be at least 1");
    if (!(M.dv > 0.0) || !finite(M.dv) || !finite(M.v0) || !finite(M.hubble)) return fail(c, FTTE_ERR_ARG, who + "dv must be positive; v0, dv and hubble finite");
    if (!(M.period >= 0.0) || !finite(M.period)) return fail(c, FTTE_ERR_ARG, who + "period must not be negative");
    const double sigma = M.line[0], damping = M.line[1], mass = M.line[2], bturb = M.line[3];
    if (!(mass > 0.0) || !finite(mass)) return fail(c, FTTE_ERR_ARG, who + "the absorber's mass must be positive");
    if (!(damping >= 0.0) || !finite(damping) || !(bturb >= 0.0) || !finite(bturb)) return fail(c, FTTE_ERR_ARG, who + "damping and b_turb must not be negative");
    if (!finite(sigma)) return fail(c, FTTE_ERR_ARG, who + "sigma_line must be finite");
    const size_t npix = (size_t)M.nxmap * (size_t)M.nymap;
    if (npix > ((size_t)1 << 30)) return fail(c, FTTE_ERR_UNSUPPORTED, who + "more than 2^30 sightlines");
    const GasState &G = c->gas;
    if (!G.ready(c->ncell)) return fail(c, FTTE_ERR_STATE, who + "no medium: call ftte_set_medium first");
    if (!c->chem.temperature_set) return fail(c, FTTE_ERR_STATE, who + "no temperature (ftte_set_temperature)");

    std::vector<int32_t> base[2];
    std::vector<double> frac[2];
    const int extent[2] = {M.nxmap, M.nymap};
    for (int a = 0; a < 2; ++a) {
        base[a].resize((size_t)extent[a]);
        frac[a].resize((size_t)extent[a]);
        if (map_axis(c->n, extent[a], M.centre[a], M.zoom, false, base[a].data(), frac[a].data()))
            return fail(c, FTTE_ERR_ARG, who + "the window leaves the box (centre, zoom)");
    }
    if (map_depth(c->n, M.centre[2], M.zoom, &R.kstart, &R.kend)) return fail(c, FTTE_ERR_ARG, who + "the window leaves the box (centre, zoom)");
    if (c->tree.max_level + 1 > kMapLevels) return fail(c, FTTE_ERR_UNSUPPORTED, who + "tree deeper than 63 levels");

    FTTE_HIP(c, hipSetDevice(c->device));
    if ((rc = wait_sweep(c))) return rc;
    SpectraState &S = c->spectra;
    FTTE_HIP(c, c->dtree.ensure(c->stream, c->tree));
    for (int a = 0; a < 2; ++a) {
        FTTE_HIP(c, S.base[a].reserve(base[a].size()));
        FTTE_HIP(c, S.frac[a].reserve(frac[a].size()));
        FTTE_HIP(c, hipMemcpyAsync(S.base[a], base[a].data(), sizeof(int32_t) * base[a].size(), hipMemcpyHostToDevice, c->stream));
        FTTE_HIP(c, hipMemcpyAsync(S.frac[a], frac[a].data(), sizeof(double) * frac[a].size(), hipMemcpyHostToDevice, c->stream));
    }
    const double *value = M.value;
    if (value && !M.on_device) {
        FTTE_HIP(c, S.value.reserve((size_t)c->ncell));
        if ((rc = upload(c, S.value, value, sizeof(double) * (size_t)c->ncell))) return rc;
        value = S.value;
    }
    if (!value) value = G.field(GasState::kHI);
    FTTE_HIP(c, S.nseg.reserve(npix));
    FTTE_HIP(c, S.column.reserve(npix));
    FTTE_HIP(c, S.flags.reserve(2));
    FTTE_HIP(c, hipMemsetAsync(S.flags, 0, 2 * sizeof(int32_t), c->stream));

    // the line of sight is the sweep frame's depth: the velocity along the storage axis that the depth feeds, against it where mirrored
    int depth_axis = 0;
    for (int a = 0; a < 3; ++a)
        if (R.zone.src[a] == 2) depth_axis = a;
    R.node = c->dtree.nodes();
    R.value = value;
    R.tgas = c->chem.tgas;
    R.vel = S.velocity_set ? S.vel[depth_axis].get() : nullptr;
    R.vel_negate = R.zone.mirror[depth_axis];
    R.ibase = S.base[0]; R.jbase = S.base[1]; R.ifrac = S.frac[0]; R.jfrac = S.frac[1];
    R.n = c->n; R.nxmap = M.nxmap; R.nymap = M.nymap;
    R.cell_cm = c->box / (double)c->n;
    R.par.v0 = M.v0; R.par.dv = M.dv; R.par.hubble = M.hubble;
    R.par.period = M.period; R.par.inv_period = M.period > 0.0 ? 1.0 / M.period : 0.0;
    R.par.sigma = sigma; R.par.damping = damping; R.par.mass = mass; R.par.bturb = bturb;
    R.K = kMath;
    R.nseg = S.nseg; R.column = S.column; R.flags = S.flags;
    R.nvel = M.nvel;

    // the pass of its own: every leaf of every sightline has a line width, or nothing of the caller's is written
    int32_t flags[2] = {0, 0};
    hipError_t e = hipSuccess;
    int lrc = launch_spectra_check(R, c->stream.get());
    if (!lrc) e = hipMemcpyAsync(flags, S.flags, sizeof flags, hipMemcpyDeviceToHost, c->stream);
    hipError_t es = hipStreamSynchronize(c->stream); // (the tables are locals)
    if (lrc) return fail(c, lrc == -1 ? FTTE_ERR_ARG : FTTE_ERR_NO_DEVICE, who + "kernel launch failed");
    if (e != hipSuccess || es != hipSuccess) return fail(c, FTTE_ERR_NO_DEVICE, who + hipGetErrorString(e != hipSuccess ? e : es));
    if (flags[0]) return fail(c, FTTE_ERR_ARG, who + "2 k_B T / mass + b_turb^2 of a leaf on a sightline is not positive and finite");

    const int64_t most = flags[1];
    const bool stage_tau = !(M.on_device && M.tau), stage_summary = M.summary && !M.on_device, spill = most > kSpectraChunk;
    const int64_t batch = spectra_batch_lines((int64_t)npix, M.nvel, stage_tau, most);
    if (stage_tau) FTTE_HIP(c, S.tau.reserve((size_t)batch * (size_t)M.nvel));
    if (stage_summary) FTTE_HIP(c, S.summary.reserve((size_t)batch * 3));
    if (spill) FTTE_HIP(c, S.spill.reserve((size_t)batch * (size_t)most));
    R.spill = spill ? S.spill.get() : nullptr;
    R.spill_stride = spill ? most : 0;
    for (int64_t line0 = 0; line0 < (int64_t)npix; line0 += batch) {
        const int64_t nl = std::min<int64_t>(batch, (int64_t)npix - line0);
        R.line0 = line0;
        R.nlines = (int32_t)nl;
        R.tau = stage_tau ? S.tau.get() : M.tau + line0 * M.nvel;
        R.summary = !M.summary ? nullptr : stage_summary ? S.summary.get() : M.summary + line0 * 3;
        if ((lrc = launch_spectra(R, c->stream.get()))) return fail(c, lrc == -1 ? FTTE_ERR_ARG : FTTE_ERR_NO_DEVICE, who + "kernel launch failed");
        if (!M.on_device) {
            if (M.tau && (rc = download(c, M.tau + line0 * M.nvel, S.tau, sizeof(double) * (size_t)nl * (size_t)M.nvel))) return rc;
            if (M.summary && (rc = download(c, M.summary + line0 * 3, S.summary, sizeof(double) * (size_t)nl * 3))) return rc;
        }
    }
    FTTE_HIP(c, hipStreamSynchronize(c->stream));
    return FTTE_OK;
}

} // namespace

extern "C" {

int ftte_set_velocity(ftte_ctx *c, const double *velx, const double *vely, const double *velz)
{
    return set_velocity(c, velx, vely, velz, false, "ftte_set_velocity");
}

int ftte_set_velocity_device(ftte_ctx *c, const double *velx_dev, const double *vely_dev, const double *velz_dev)
{
    return set_velocity(c, velx_dev, vely_dev, velz_dev, true, "ftte_set_velocity_device");
}

int ftte_sightline_spectra(ftte_ctx *c, int izone, int nxmap, int nymap, const double *centre, double zoom, int nvel, double v0, double dv,
                           double hubble, double period, const double *line, const double *value, double *tau, double *summary)
{
    return make_spectra(c, SpectraCall{"ftte_sightline_spectra", izone, nxmap, nymap, centre, zoom, nvel, v0, dv, hubble, period, line, value, false, tau, summary});
}

int ftte_sightline_spectra_device(ftte_ctx *c, int izone, int nxmap, int nymap, const double *centre, double zoom, int nvel, double v0, double dv,
                                  double hubble, double period, const double *line, const double *value_dev, double *tau_dev, double *summary_dev)
{
    return make_spectra(c, SpectraCall{"ftte_sightline_spectra_device", izone, nxmap, nymap, centre, zoom, nvel, v0, dv, hubble, period, line, value_dev, true, tau_dev,
                                       summary_dev});
}

} // extern "C"
