// ftte_api.cpp -- the C ABI of include/ftte.h: context life cycle, grid and field setters, options, the sweep entry points, point
// sources, host helpers; the entry points that read or write the species medium are in ftte_chem.cpp.  The work behind them:
// ftte_plan.cpp (planners), ftte_sweeps.cpp (launch sequences), ftte_hybrid.cpp (refined cell arrays), ftte_host_arrays.cpp (PCIe),
// ftte_point.cpp, ftte_tables.cpp (the reference's table mathematics), ftte_amr.cpp, ftte_ingest.cpp.
//
// There is no CPU fallback: every entry point that computes on the grid needs a HIP device and fails with FTTE_ERR_NO_DEVICE
// otherwise.
#include "ftte_context.h"

using namespace ftte;

namespace ftte {

std::string g_create_error;

int fail(ftte_ctx *c, int code, const std::string &msg)
{
    if (c) c->err = msg;
    else g_create_error = msg;
    return code;
}

int check_single(ftte_ctx *c)
{
    if (c && c->multi) return check_ready(c, false); // (refuses: a multi-device context routes the diffuse sweep only)
    return c ? FTTE_OK : FTTE_ERR_ARG;
}

} // namespace ftte


// =================================================================================================
extern "C" {

int ftte_create(ftte_ctx **out, int ndev, const int *dev_ids)
{
    if (!out) return fail(nullptr, FTTE_ERR_ARG, "ftte_create: ctx is NULL");
    *out = nullptr;
    if (ndev > 1) return multi_create(out, ndev, dev_ids); // one single-device context per device behind this one (ftte_multi.cpp)
    if (ndev != 1) return fail(nullptr, FTTE_ERR_ARG, "ftte_create: ndev must be at least 1");
    int count = 0;
    hipError_t e = hipGetDeviceCount(&count);
    if (e != hipSuccess || count <= 0)
        return fail(nullptr, FTTE_ERR_NO_DEVICE, std::string("ftte_create: no HIP device (") +
                                                     (e != hipSuccess ? hipGetErrorString(e) : "device count is 0") + ")");
    int dev = 0;
    if (dev_ids) dev = dev_ids[0];
    else if (hipGetDevice(&dev) != hipSuccess) dev = 0;
    if (dev < 0 || dev >= count) return fail(nullptr, FTTE_ERR_ARG, "ftte_create: device ordinal out of range");
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, dev) != hipSuccess) return fail(nullptr, FTTE_ERR_NO_DEVICE, "hipGetDeviceProperties failed");
    if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0)
        return fail(nullptr, FTTE_ERR_NO_DEVICE, std::string("ftte_create: kernels are built for gfx950 only, device is ") + prop.gcnArchName);
    ftte_ctx *c = new ftte_ctx;
    c->device = dev;
    if (hipSetDevice(dev) != hipSuccess || c->stream.create(hipStreamDefault) != hipSuccess) {
        delete c;
        return fail(nullptr, FTTE_ERR_NO_DEVICE, "ftte_create: cannot create a stream on the device");
    }
    *out = c;
    return FTTE_OK;
}

int ftte_destroy(ftte_ctx *c)
{
    if (!c) return FTTE_ERR_ARG;
    if (c->multi) return multi_destroy(c);
    (void)hipSetDevice(c->device);
    if (c->stream) (void)hipStreamSynchronize(c->stream);
    delete c;
    return FTTE_OK;
}

const char *ftte_last_error(const ftte_ctx *c) { return c ? c->err.c_str() : g_create_error.c_str(); }

const char *ftte_multi_info(const ftte_ctx *c) { return (c && c->multi) ? multi_how(c) : ""; }

int ftte_set_grid(ftte_ctx *c, int nx, int ny, int nz, int64_t ncell, const int32_t *level, double box_cm)
{
    if (!c) return FTTE_ERR_ARG;
    if (nx < 1 || !level || ncell < 1 || !(box_cm > 0.0)) return fail(c, FTTE_ERR_ARG, "ftte_set_grid: bad argument");
    if (nx != ny || nx != nz) return fail(c, FTTE_ERR_NOT_CUBIC, "base grid needs to be of size n^3");
    if (nx > 32000) return fail(c, FTTE_ERR_UNSUPPORTED, "ftte_set_grid: n > 32000");
    if (c->multi) return multi_set_grid(c, nx, ny, nz, ncell, level, box_cm);
    // The reference's tree is static over a run while its driver would hand the same list over on every outer iteration
    // (the drop-ins do): an unchanged list keeps the tree, the sweep plan, the segment forests and the resident medium.
    // Only the box may differ (the plans are keyed on it themselves).
    if (c->grid_set && c->n == nx && c->ncell == ncell && (int64_t)c->leaf_level.size() == ncell) {
        bool same = true;
        const int8_t *have = c->leaf_level.data();
        for (int64_t q = 0; q < ncell; ++q)
            if ((int32_t)have[q] != level[q]) { same = false; break; }
        if (same) { c->box = box_cm; return FTTE_OK; }
    }
    // rebuild the tree exactly as createFullyThreadedStructure does (readCellArray.f90:154-187); this also
    // validates the list
    ++c->n_grid_builds;
    if (c->sweep_pending) { (void)hipSetDevice(c->device); (void)hipEventSynchronize(c->ev_sweep_done); c->sweep_pending = false; }
    AmrTree tree;
    const std::string terr = tree.build(nx, ncell, level);
    if (!terr.empty()) return fail(c, FTTE_ERR_LEVELS, terr);
    if (tree.refined() && 3 * ncell >= (int64_t)1 << 31) return fail(c, FTTE_ERR_UNSUPPORTED, "refined cell array with more than 7.1e8 leaves");
    if (c->grid_set && (c->n != nx || c->ncell != ncell)) {
        // a different grid: drop everything sized by the old one
        (void)hipSetDevice(c->device);
        (void)hipStreamSynchronize(c->stream);
        c->kappa.release(); c->emis.release();
        for (auto &layout : c->acc)
            for (auto &a : layout) a.reset();
        c->emit_mode = 0;
        c->fscratch.drop();
        c->nnu = 0;
    }
    (void)hipSetDevice(c->device);
    (void)hipStreamSynchronize(c->stream);
    c->forests.drop();
    c->hplan = HybridPlan();
    c->hdev.drop_grid();
    c->gas.drop();
    c->point.drop_grid();
    c->catalogue.drop_grid();
    c->dtree.drop();
    c->chem.drop_grid();
    c->analysis.drop_grid();
    c->spectra.drop_grid();
    c->leaf_level.assign(level, level + ncell);
    c->n = nx; c->ncell = ncell; c->box = box_cm; c->grid_set = true;
    c->kappa.invalidate();
    c->plan.valid = false;
    c->bplan.valid = false;
    c->tree = std::move(tree);
    return FTTE_OK;
}

int ftte_set_opacity(ftte_ctx *c, int nnu, const double *kappa)
{
    if (c && c->multi) return multi_set_opacity(c, nnu, kappa);
    int rc = check_ready(c, false);
    if (rc) return rc;
    if (nnu < 1 || !kappa) return fail(c, FTTE_ERR_ARG, "ftte_set_opacity: bad argument");
    FTTE_HIP(c, hipSetDevice(c->device));
    if ((rc = wait_sweep(c))) return rc;
    FTTE_HIP(c, hipStreamSynchronize(c->stream));
    if ((rc = ensure_kappa(c, nnu))) return rc;
    if ((rc = upload(c, c->kappa.source(), kappa, sizeof(double) * nnu * c->ncell))) return rc;
    c->nnu = nnu;
    c->kappa.set();
    return FTTE_OK;
}

int ftte_set_opacity_device(ftte_ctx *c, int nnu, const double *kappa_dev)
{
    int rc = check_ready(c, false);
    if (rc) return rc;
    if (nnu < 1 || !kappa_dev) return fail(c, FTTE_ERR_ARG, "ftte_set_opacity_device: bad argument");
    FTTE_HIP(c, hipSetDevice(c->device));
    if ((rc = wait_sweep(c))) return rc;
    if ((rc = ensure_kappa(c, nnu))) return rc;
    // A uniform grid whose last sweep used the transposed layout 2 (the copy is there): the copy and the transposes in one pass over
    // the caller's array, layout 1 too where the last sweep used it (the tile engine; the brick engine marches layout 1 through
    // layout 0).  Else the copy alone; the sweep makes what it needs.
    const bool same = !c->use_forest() && c->nnu == nnu && !c->opt.launch.tiled;
    const bool with2 = same && c->kappa.current(MediumField::kLayout2), with1 = with2 && c->kappa.current(MediumField::kLayout1);
    if (with2) {
        if (launch_set_layouts(kappa_dev, c->kappa.source(), with1 ? c->kappa.in_layout(1) : nullptr, c->kappa.in_layout(2), c->n, nnu, (long)c->ncell, c->stream))
            return fail(c, FTTE_ERR_NO_DEVICE, "layout kernel launch failed");
    } else FTTE_HIP(c, hipMemcpyAsync(c->kappa.source(), kappa_dev, sizeof(double) * nnu * c->ncell, hipMemcpyDeviceToDevice, c->stream));
    FTTE_HIP(c, hipStreamSynchronize(c->stream)); // the sweep may run on another stream: the copies must have landed
    c->nnu = nnu;
    c->kappa.set();
    if (with2) c->kappa.made(MediumField::kLayout2); // written in the same pass
    if (with1) c->kappa.made(MediumField::kLayout1);
    return FTTE_OK;
}

int ftte_set_species(ftte_ctx *c, int nnu, const double *HI, const double *HeI, const double *HeII, const double *beta)
{
    int rc = check_ready(c, false);
    if (rc) return rc;
    if (nnu < 1 || !HI || !HeI || !HeII || !beta) return fail(c, FTTE_ERR_ARG, "ftte_set_species: bad argument");
    FTTE_HIP(c, hipSetDevice(c->device));
    if ((rc = wait_sweep(c))) return rc;
    FTTE_HIP(c, hipStreamSynchronize(c->stream));
    if ((rc = ensure_kappa(c, nnu))) return rc;
    DeviceBuffer<double> tmp;
    const size_t nc = (size_t)c->ncell;
    FTTE_HIP(c, tmp.reserve(3 * nc + 3 * (size_t)nnu));
    hipError_t e = hipMemcpyAsync(tmp, HI, sizeof(double) * nc, hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(tmp + nc, HeI, sizeof(double) * nc, hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(tmp + 2 * nc, HeII, sizeof(double) * nc, hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(tmp + 3 * nc, beta, sizeof(double) * 3 * nnu, hipMemcpyHostToDevice, c->stream);
    int lrc = 0;
    if (e == hipSuccess) lrc = launch_opacity(tmp, tmp + nc, tmp + 2 * nc, tmp + 3 * nc, c->kappa.source(), (long)nc, nnu, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e != hipSuccess) return fail(c, FTTE_ERR_NO_DEVICE, std::string("ftte_set_species: ") + hipGetErrorString(e));
    if (lrc) return fail(c, FTTE_ERR_NO_DEVICE, "ftte_set_species: kernel launch failed");
    c->nnu = nnu;
    c->kappa.set();
    return FTTE_OK;
}

static int set_emission(ftte_ctx *c, int mode, const double *values, bool on_device, const char *who)
{
    if (!c) return FTTE_ERR_ARG;
    if (c->multi) return on_device ? fail(c, FTTE_ERR_UNSUPPORTED, std::string(who) + ": a multi-device context takes host arrays") : multi_set_emission(c, mode, values);
    if (!values) { c->emit_mode = 0; return FTTE_OK; }
    int rc = check_ready(c, true);
    if (rc) return rc;
    FTTE_HIP(c, hipSetDevice(c->device));
    if ((rc = wait_sweep(c))) return rc;
    if (!on_device) FTTE_HIP(c, hipStreamSynchronize(c->stream));
    FTTE_HIP(c, c->emis.reserve_source(c->kappa.capacity()));
    const size_t bytes = sizeof(double) * (size_t)c->nnu * c->ncell;
    FTTE_HIP(c, hipMemcpyAsync(c->emis.source(), values, bytes, on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, c->stream));
    FTTE_HIP(c, hipStreamSynchronize(c->stream)); // the sweep may run on another stream: the copy must have landed
    c->emit_mode = mode;
    c->emis.set();
    (void)who;
    return FTTE_OK;
}

int ftte_set_emissivity(ftte_ctx *c, const double *eta) { return set_emission(c, 1, eta, false, "ftte_set_emissivity"); }
int ftte_set_emissivity_device(ftte_ctx *c, const double *eta_dev) { return set_emission(c, 1, eta_dev, true, "ftte_set_emissivity_device"); }
int ftte_set_source_function(ftte_ctx *c, const double *S) { return set_emission(c, 2, S, false, "ftte_set_source_function"); }
int ftte_set_source_function_device(ftte_ctx *c, const double *S_dev) { return set_emission(c, 2, S_dev, true, "ftte_set_source_function_device"); }

int ftte_set_option(ftte_ctx *c, const char *key, int value)
{
    if (!c || !key) return FTTE_ERR_ARG;
    if (c->multi) return multi_set_option(c, key, value);
    std::string why;
    const OptionSet how = set(c->opt, key, value, &why); // ranges, refusals and where the value goes: the table of ftte_options.h
    if (how == OptionSet::refused) return fail(c, FTTE_ERR_ARG, why);
    if (how == OptionSet::stored_invalidate) { // (also where the value did not change)
        c->plan.valid = c->bplan.valid = false;
        c->hplan.invalidate();
    }
    return FTTE_OK;
}

int ftte_diffuse_sweep_device(ftte_ctx *c, int ndir, const double *phi, const double *theta, const double *w,
                              const double *uvb, double *J_dev, void *stream_v)
{
    int rc = check_ready(c, true);
    if (rc) return rc;
    if (ndir < 0 || (ndir > 0 && (!phi || !theta || !w)) || !uvb || !J_dev)
        return fail(c, FTTE_ERR_ARG, "ftte_diffuse_sweep: bad argument");
    FTTE_HIP(c, hipSetDevice(c->device));
    hipStream_t stream = stream_v ? (hipStream_t)stream_v : c->stream;

    if (c->use_forest()) {
        if (c->opt.hybrid.hybrid && c->tree.refined() && !c->opt.route.forest && ndir > 0) {
            bool done = false;
            if ((rc = hybrid_sweep(c, ndir, phi, theta, w, uvb, J_dev, stream, &done)) || done) return rc;
        }
        return forest_sweep(c, ndir, phi, theta, w, uvb, J_dev, stream);
    }
    if (c->opt.route.engine != 1) return brick_sweep(c, ndir, phi, theta, w, uvb, J_dev, stream);
    return tile_sweep(c, ndir, phi, theta, w, uvb, J_dev, stream);
}

int ftte_diffuse_sweep(ftte_ctx *c, int ndir, const double *phi, const double *theta, const double *w, const double *uvb,
                       double *J)
{
    if (c && c->multi) return multi_sweep(c, ndir, phi, theta, w, uvb, J);
    int rc = check_ready(c, true);
    if (rc) return rc;
    if (!J) return fail(c, FTTE_ERR_ARG, "ftte_diffuse_sweep: J is NULL");
    FTTE_HIP(c, hipSetDevice(c->device));
    const size_t elems = (size_t)c->nnu * c->ncell;
    FTTE_HIP(c, c->host.J_dev.reserve(elems)); // kept from call to call
    if ((rc = ftte_diffuse_sweep_device(c, ndir, phi, theta, w, uvb, c->host.J_dev, nullptr))) return rc;
    if ((rc = download(c, J, c->host.J_dev, sizeof(double) * elems))) return rc;
    return wait_sweep(c); // the sweep has drained: report a dataflow sweep that gave up now rather than at the next call
}

/* ftte_set_opacity + ftte_diffuse_sweep in one call, and faster than the two: on a uniform grid swept by the brick engine the
 * frequency groups travel in lanes (option "lanes") -- the first lane is swept while the second one's opacities are still
 * crossing PCIe, and its J goes back while the second is swept.  Same results; elsewhere the two calls one after the other. */
int ftte_diffuse_iteration(ftte_ctx *c, int nnu, const double *kappa, int ndir, const double *phi, const double *theta, const double *w,
                           const double *uvb, double *J)
{
    if (c && c->multi) return multi_iteration(c, nnu, kappa, ndir, phi, theta, w, uvb, J);
    int rc = check_ready(c, false);
    if (rc) return rc;
    if (nnu < 1 || !kappa || !J || ndir < 0 || (ndir > 0 && (!phi || !theta || !w)) || !uvb)
        return fail(c, FTTE_ERR_ARG, "ftte_diffuse_iteration: bad argument");
    const BrickOptions &B = c->opt.brick;
    const bool lanes_apply = !c->use_forest() && c->opt.route.engine != 1 && !c->emit_mode && B.brick_form(nnu, c->emit_mode) != 1 && !B.dataflow && ndir > 0 &&
                             B.lanes >= 2 && nnu >= B.lanes;
    if (!lanes_apply) {
        if ((rc = ftte_set_opacity(c, nnu, kappa))) return rc;
        return ftte_diffuse_sweep(c, ndir, phi, theta, w, uvb, J);
    }
    FTTE_HIP(c, hipSetDevice(c->device));
    if ((rc = wait_sweep(c))) return rc;
    FTTE_HIP(c, hipStreamSynchronize(c->stream));
    if ((rc = ensure_kappa(c, nnu))) return rc;
    c->nnu = nnu;
    c->kappa.invalidate(); // the lanes bring it: set() when the last one has been issued (brick_sweep)
    const size_t elems = (size_t)nnu * c->ncell;
    FTTE_HIP(c, c->host.J_dev.reserve(elems));
    const HostPipe pipe{kappa, J};
    if ((rc = brick_sweep(c, ndir, phi, theta, w, uvb, c->host.J_dev, c->stream, &pipe))) {
        c->kappa.invalidate();
        return rc;
    }
    return wait_sweep(c); // J is in the caller's array on return
}

/* Pins a caller-owned host array for as long as it stays registered: ftte_set_opacity / ftte_diffuse_sweep then move
 * it by DMA directly (no staging copy).  The caller unregisters it before freeing it. */
int ftte_host_register(ftte_ctx *c, void *ptr, size_t bytes)
{
    if (!c) return FTTE_ERR_ARG;
    if (!ptr || !bytes) return fail(c, FTTE_ERR_ARG, "ftte_host_register: bad argument");
    if (c->multi) return multi_host_register(c, ptr, bytes, true);
    FTTE_HIP(c, hipSetDevice(c->device));
    FTTE_HIP(c, c->host.pin(ptr, bytes));
    return FTTE_OK;
}

int ftte_host_unregister(ftte_ctx *c, void *ptr)
{
    if (!c) return FTTE_ERR_ARG;
    if (c->multi) return multi_host_register(c, ptr, 0, false);
    if (!c->host.pinned(ptr)) return fail(c, FTTE_ERR_ARG, "ftte_host_unregister: not a registered array");
    FTTE_HIP(c, hipSetDevice(c->device));
    FTTE_HIP(c, hipStreamSynchronize(c->stream));
    FTTE_HIP(c, c->host.unpin(ptr));
    return FTTE_OK;
}

long long ftte_counter(const ftte_ctx *c, const char *name)
{
    if (!c || !name) return -1;
    if (c->multi) return multi_counter(c, name);
    if (!std::strcmp(name, "devices")) return 1;
    if (!std::strcmp(name, "grid_builds")) return c->n_grid_builds;
    if (!std::strcmp(name, "plan_builds")) return c->n_plan_builds;
    if (!std::strcmp(name, "forest_builds")) return c->n_forest_builds;
    if (!std::strcmp(name, "device_objects")) return g_device_objects.load();
    if (!std::strcmp(name, "spectra_chunk_segments")) return kSpectraChunk;     // segments of a sightline in LDS at a time
    if (!std::strcmp(name, "spectra_pass_pixels")) return kSpectraPassPixels;   // pixels of a sightline a workgroup holds in registers in one pass
    if (!std::strcmp(name, "spectra_velocity")) return c->spectra.velocity_set ? 1 : 0;
    if (!std::strcmp(name, "ray_chunk_segments")) return kSpectraChunk;         // records of a ray in LDS at a time (ftte_rays.hip)
    if (!std::strcmp(name, "ray_work_bytes")) return (long long)kSpectraWorkBytes; // what a batch of rays keeps stays below this
    if (!std::strcmp(name, "population_slots")) return c->point.tables.slot_count();
    if (!std::strcmp(name, "expansion_exact_tests")) return c->chem.expansion_tests;
    if (!std::strcmp(name, "medium_abun2")) return c->gas.ready_with_abundance(c->ncell) ? 1 : 0; // the medium came with an abun2
    if (!std::strcmp(name, "catalogue_stars")) return c->catalogue.stars();      // of the last ftte_star_catalogue
    if (!std::strcmp(name, "catalogue_sources")) return c->catalogue.sources();  // -1: there is none
    if (!std::strncmp(name, "catalogue_ns_", 13)) { // device time of the last catalogue's launches: locate, count, scan, emit
        static const char *const phase[4] = {"locate", "count", "scan", "emit"};
        for (int p = 0; p < 4; ++p)
            if (!std::strcmp(name + 13, phase[p])) return catalogue_phase_ns(c->catalogue, p);
        return -1;
    }
    if (!std::strcmp(name, "hybrid_boxes")) return c->hplan.boxes();
    if (!std::strcmp(name, "hybrid_passes")) return c->hplan.passes();
    if (!std::strcmp(name, "fine_block")) return c->hplan.fine_block();
    if (!std::strcmp(name, "brick_form")) return c->last_brick_form;
    if (!std::strcmp(name, "brick_dataflow")) return c->last_brick_dataflow;
    if (!std::strcmp(name, "brick_whole")) return c->last_brick_whole; // 1: the last sweep's stage launches took the whole-brick form
    if (!std::strcmp(name, "brick_duo")) return c->last_brick_duo;     // seats of the last sweep's plan where two passes share a visit (0: single passes)
    if (!std::strcmp(name, "nu_deal")) return c->opt.launch.nu_deal; // the option as it stands (its default before anybody set it)
    if (!std::strcmp(name, "brick_chunk")) return c->bplan.valid ? c->bplan.chunk : 0;
    if (!std::strcmp(name, "brick_queue_mix")) return (c->bplan.valid && c->bplan.persistent) ? c->bplan.key.queue_mix : -1;
    if (!std::strcmp(name, "brick_groups")) return c->bplan.valid ? (long long)c->bplan.groups.size() : 0;
    if (!std::strcmp(name, "brick_accumulators")) return c->bplan.valid ? c->bplan.nacc[0] + c->bplan.nacc[1] + c->bplan.nacc[2] : 0;
    if (!std::strcmp(name, "brick_accumulators_0")) return c->bplan.valid ? c->bplan.nacc[0] : 0;
    if (!std::strcmp(name, "brick_accumulators_1")) return c->bplan.valid ? c->bplan.nacc[1] : 0;
    if (!std::strcmp(name, "brick_accumulators_2")) return c->bplan.valid ? c->bplan.nacc[2] : 0;
    if (!std::strcmp(name, "brick_stages")) return c->bplan.valid ? c->bplan.nstages : 0;
    if (!std::strcmp(name, "merge_points")) return c->bplan.valid ? (long long)c->bplan.merge_stage.size() : 0;
    if (!std::strcmp(name, "merge_blocks")) return c->bplan.valid ? (long long)c->bplan.merge_blocks.size() : 0;
    if (!std::strncmp(name, "merge_stage_", 12) || !std::strncmp(name, "merge_final_", 12)) { // merge point k: its stage, blocks final by then
        char *end = nullptr;
        const long k = std::strtol(name + 12, &end, 10);
        if (!c->bplan.valid || end == name + 12 || *end || k < 0 || k >= (long)c->bplan.merge_stage.size()) return -1;
        return name[6] == 's' ? c->bplan.merge_stage[(size_t)k] : (long long)c->bplan.merge_off[(size_t)k + 1];
    }
    return -1;
}

int ftte_launch_count(const ftte_ctx *c) { return !c ? 0 : c->multi ? multi_first(c)->timing_used : c->timing_used; }

int ftte_launch_info(ftte_ctx *c, int idx, double *ms, int64_t *updates)
{
    if (c && c->multi) return ftte_launch_info(multi_first(c), idx, ms, updates); // (the first device's share of the sweep)
    if (!c || idx < 0 || idx >= c->timing_used) return FTTE_ERR_ARG;
    float t = 0.f;
    const LaunchTiming &T = c->timing[idx];
    if (T.lanes > 0) {
        float begin = 0.f, end = 0.f;
        for (int l = 0; l < T.lanes; ++l) {
            float b = 0.f, e = 0.f;
            FTTE_HIP(c, hipEventElapsedTime(&b, T.start, T.first[(size_t)l]));
            FTTE_HIP(c, hipEventElapsedTime(&e, T.start, T.last[(size_t)l]));
            begin = l ? std::min(begin, b) : b;
            end = l ? std::max(end, e) : e;
        }
        t = end - begin;
    } else FTTE_HIP(c, hipEventElapsedTime(&t, T.start, T.stop));
    if (ms) *ms = t;
    if (updates) *updates = c->timing[idx].updates;
    return FTTE_OK;
}

// ---- host geometry ----------------------------------------------------------------------------------
int ftte_rotate_indices(int i, int j, int k, int nx, int ny, int nz, int izone, int *ic, int *jc, int *kc)
{
    if (!ic || !jc || !kc) return FTTE_ERR_ARG;
    return rotate_indices(i, j, k, nx, ny, nz, izone, ic, jc, kc) ? FTTE_ERR_IZONE : FTTE_OK;
}

int ftte_pix2ang_nest(int nside, int64_t ipix, double *phi, double *theta)
{
    if (!phi || !theta) return FTTE_ERR_ARG;
    return pix2ang_nest(nside, ipix, phi, theta) ? FTTE_ERR_PIXEL : FTTE_OK;
}

int ftte_fold_direction(double phi_large, double theta_large, double *phi, double *theta, int *izone)
{
    if (!phi || !theta || !izone) return FTTE_ERR_ARG;
    const int rc = fold_direction(phi_large, theta_large, phi, theta, izone);
    return rc ? fold_status(rc) : FTTE_OK;
}

int ftte_set_pattern(ftte_pattern *pattern, double phi, double theta)
{
    if (!pattern) return FTTE_ERR_ARG;
    return set_pattern(pattern, phi, theta) ? FTTE_ERR_PATTERN : FTTE_OK;
}

int ftte_layer_patterns(int n, double phi, double theta, ftte_pattern *layers)
{
    if (n < 1 || !layers) return FTTE_ERR_ARG;
    return layer_patterns(n, phi, theta, layers) ? FTTE_ERR_PATTERN : FTTE_OK;
}

void ftte_compute_cell_intensity(double *Jmean, double Iin, double Iout)
{
    // transportRoutinesModule.f90:1044-1048, the reference's own formula (host helper; the device
    // evaluates the same mean through ftte_math.h)
    if (Iout < Iin) *Jmean += (Iin - Iout) / std::log(Iin / Iout);
    else *Jmean += 0.5 * (Iin + Iout);
}

// ---- point sources --------------------------------------------------------------------------------------------

int ftte_stellar_beta_table(ftte_ctx *c, const double *a_smc, int nwave, const double *wavelength_cm, int nspectrum, int nmetal,
                            const double *specific_luminosity, int iSpectrum, double coefSpectrum, int iMetal, double coefMetal,
                            double *total_integral)
{
    int rc = check_single(c);
    if (rc) return rc;
    if (!a_smc || !wavelength_cm || !specific_luminosity || nwave < 2 || nspectrum < 2 || nmetal < 2)
        return fail(c, FTTE_ERR_ARG, "ftte_stellar_beta_table: bad argument");
    if (iSpectrum < 1 || iSpectrum + 1 > nspectrum || iMetal < 1 || iMetal + 1 > nmetal)
        return fail(c, FTTE_ERR_ARG, "ftte_stellar_beta_table: iSpectrum / iMetal outside the library");
    FTTE_HIP(c, hipSetDevice(c->device));
    return point_stellar_beta_table(c->point.tables, c->stream, a_smc, nwave, wavelength_cm, nspectrum, nmetal, specific_luminosity, iSpectrum,
                                    coefSpectrum, iMetal, coefMetal, total_integral, &c->err);
}

int ftte_stellar_beta_tables(ftte_ctx *c, const double *a_smc, int nwave, const double *wavelength_cm, int nspectrum, int nmetal,
                             const double *specific_luminosity, int npop, const int *iSpectrum, const double *coefSpectrum,
                             const int *iMetal, const double *coefMetal, double *total_integral)
{
    int rc = check_single(c);
    if (rc) return rc;
    if (!a_smc || !wavelength_cm || !specific_luminosity || nwave < 2 || nspectrum < 2 || nmetal < 2 || npop < 1 || !iSpectrum ||
        !coefSpectrum || !iMetal || !coefMetal)
        return fail(c, FTTE_ERR_ARG, "ftte_stellar_beta_tables: bad argument");
    for (int p = 0; p < npop; ++p)
        if (iSpectrum[p] < 1 || iSpectrum[p] + 1 > nspectrum || iMetal[p] < 1 || iMetal[p] + 1 > nmetal)
            return fail(c, FTTE_ERR_ARG, "ftte_stellar_beta_tables: iSpectrum / iMetal of population " + std::to_string(p) + " outside the library");
    FTTE_HIP(c, hipSetDevice(c->device));
    return point_stellar_beta_tables(c->point.tables, c->stream, a_smc, nwave, wavelength_cm, nspectrum, nmetal, specific_luminosity, npop,
                                     iSpectrum, coefSpectrum, iMetal, coefMetal, total_integral, &c->err);
}

int ftte_set_population_tables(ftte_ctx *c, int npop, const double *tables)
{
    int rc = check_single(c);
    if (rc) return rc;
    if (npop < 1 || !tables) return fail(c, FTTE_ERR_ARG, "ftte_set_population_tables: bad argument");
    FTTE_HIP(c, hipSetDevice(c->device));
    return c->point.tables.set_slots(c->stream, npop, tables, &c->err);
}

int ftte_get_population_tables(ftte_ctx *c, int slot, double *tables)
{
    int rc = check_single(c);
    if (rc) return rc;
    if (!tables) return fail(c, FTTE_ERR_ARG, "ftte_get_population_tables: bad argument");
    const RateTables &R = c->point.tables;
    if ((rc = R.missing(true, &c->err))) return rc;
    const int count = R.slot_count();
    if (slot < 0 || slot >= count)
        return fail(c, FTTE_ERR_ARG, "ftte_get_population_tables: slot " + std::to_string(slot) + " outside 0.." + std::to_string(count - 1));
    FTTE_HIP(c, hipSetDevice(c->device));
    return R.get(c->stream, true, slot, tables, &c->err);
}

int ftte_set_rate_tables(ftte_ctx *c, const double *tables)
{
    int rc = check_single(c);
    if (rc) return rc;
    if (!tables) return fail(c, FTTE_ERR_ARG, "ftte_set_rate_tables: bad argument");
    FTTE_HIP(c, hipSetDevice(c->device));
    return c->point.tables.set_current(c->stream, tables, &c->err);
}

int ftte_get_rate_tables(ftte_ctx *c, double *tables)
{
    int rc = check_single(c);
    if (rc) return rc;
    if (!tables) return fail(c, FTTE_ERR_ARG, "ftte_get_rate_tables: bad argument");
    if ((rc = c->point.tables.missing(false, &c->err))) return rc;
    FTTE_HIP(c, hipSetDevice(c->device));
    return c->point.tables.get(c->stream, false, 0, tables, &c->err);
}

int ftte_get_rates_hydrogen_helium(ftte_ctx *c, int dust_approximation, int nsample, const double *tau, double *rates)
{
    int rc = check_single(c);
    if (rc) return rc;
    if (nsample < 0 || (nsample && (!tau || !rates)) || dust_approximation < 0 || dust_approximation > 2)
        return fail(c, FTTE_ERR_ARG, "ftte_get_rates_hydrogen_helium: bad argument");
    if (!nsample) return FTTE_OK;
    FTTE_HIP(c, hipSetDevice(c->device));
    return point_lookup(c->point, c->stream, dust_approximation, nsample, tau, rates, &c->err);
}

static int set_medium(ftte_ctx *c, const double *HI, const double *HeI, const double *HeII, const double *rho, const double *abun2,
                      int dust, bool on_device, const char *who)
{
    int rc = check_ready(c, false);
    if (rc) return rc;
    if (!HI || !HeI || !HeII || dust < 0 || dust > 2) return fail(c, FTTE_ERR_ARG, std::string(who) + ": bad argument");
    if ((dust >= 1 && !abun2) || (dust == 2 && !rho)) return fail(c, FTTE_ERR_ARG, std::string(who) + ": this dust approximation needs abun2 (and rho)");
    FTTE_HIP(c, hipSetDevice(c->device));
    const double *const field[5] = {HI, HeI, HeII, rho, abun2};
    return point_set_medium(c->gas, c->stream, c->ncell, field, on_device, dust, &c->err);
}

int ftte_set_medium(ftte_ctx *c, const double *HI, const double *HeI, const double *HeII, const double *rho, const double *abun2,
                    int dust_approximation)
{
    return set_medium(c, HI, HeI, HeII, rho, abun2, dust_approximation, false, "ftte_set_medium");
}

int ftte_set_medium_device(ftte_ctx *c, const double *HI, const double *HeI, const double *HeII, const double *rho,
                           const double *abun2, int dust_approximation)
{
    return set_medium(c, HI, HeI, HeII, rho, abun2, dust_approximation, true, "ftte_set_medium_device");
}

int ftte_set_zero_rates(ftte_ctx *c)
{
    int rc = check_ready(c, false);
    if (rc) return rc;
    FTTE_HIP(c, hipSetDevice(c->device));
    if ((rc = c->point.rates.zero(c->stream, c->ncell, &c->err))) return rc;
    FTTE_HIP(c, hipStreamSynchronize(c->stream));
    return FTTE_OK;
}

int ftte_locate_cell(ftte_ctx *c, int level, const int32_t *position, int64_t *cell)
{
    int rc = check_ready(c, false);
    if (rc) return rc;
    if (level < 0 || !position || !cell) return fail(c, FTTE_ERR_ARG, "ftte_locate_cell: bad argument");
    const int n = c->n;
    for (int q = 0; q < 3; ++q)
        if (position[q] < 1 || position[q] > n) return fail(c, FTTE_ERR_ARG, "ftte_locate_cell: base index outside 1..n");
    int32_t node = ((position[0] - 1) * n + (position[1] - 1)) * n + (position[2] - 1);
    for (int l = 0; l < level; ++l) {
        // localizeCellFromStar, equiSources.f90:2597-2620
        if (c->tree.child0[node] < 0) return fail(c, FTTE_ERR_LEVELS, "error in star particle position: cell not refined");
        const int32_t *p = position + 3 * l + 3;
        for (int q = 0; q < 3; ++q)
            if (p[q] < 1 || p[q] > 2) return fail(c, FTTE_ERR_ARG, "ftte_locate_cell: child index outside 1..2");
        node = c->tree.child0[node] + 4 * (p[0] - 1) + 2 * (p[1] - 1) + (p[2] - 1);
    }
    if (c->tree.leaf[node] < 0) return fail(c, FTTE_ERR_LEVELS, "ftte_locate_cell: the call sequence ends on a refined cell");
    *cell = c->tree.leaf[node];
    return FTTE_OK;
}

int ftte_point_sources(ftte_ctx *c, int nsrc, const int64_t *src_cell, const double *src_ndot, int *highest_pixel_level)
{
    int rc = check_ready(c, false);
    if (rc) return rc;
    if (nsrc < 0 || (nsrc && (!src_cell || !src_ndot))) return fail(c, FTTE_ERR_ARG, "ftte_point_sources: bad argument");
    if (highest_pixel_level) *highest_pixel_level = 0;
    if (!nsrc) return FTTE_OK;
    FTTE_HIP(c, hipSetDevice(c->device));
    return point_trace(c->point, c->dtree, c->gas, c->stream, c->tree, c->box, nsrc, src_cell, src_ndot, nullptr, highest_pixel_level, nullptr, &c->err);
}

int ftte_point_sources_populations(ftte_ctx *c, int nsrc, const int64_t *src_cell, const double *src_ndot, const int32_t *src_slot,
                                   int *highest_pixel_level)
{
    int rc = check_ready(c, false);
    if (rc) return rc;
    if (nsrc < 0 || (nsrc && (!src_cell || !src_ndot || !src_slot))) return fail(c, FTTE_ERR_ARG, "ftte_point_sources_populations: bad argument");
    if ((rc = c->point.tables.missing(true, &c->err))) return rc;
    if (highest_pixel_level) std::fill(highest_pixel_level, highest_pixel_level + nsrc, 0);
    if (!nsrc) return FTTE_OK;
    FTTE_HIP(c, hipSetDevice(c->device));
    return point_trace(c->point, c->dtree, c->gas, c->stream, c->tree, c->box, nsrc, src_cell, src_ndot, src_slot, nullptr, highest_pixel_level, &c->err);
}

int ftte_point_escape(ftte_ctx *c, int nsrc, double *remaining, double *boundary, double *dust, double *spectrum, double *fraction)
{
    int rc = check_single(c);
    if (rc) return rc;
    const EscapeRecord &E = c->point.escape;
    if (nsrc != E.stars())
        return fail(c, FTTE_ERR_ARG, "ftte_point_escape: nsrc is not the number of stars of the last ftte_point_sources");
    for (int s = 0; s < nsrc; ++s) E.unpack(s, remaining, boundary, dust, spectrum, fraction);
    return FTTE_OK;
}

int ftte_set_output_sigma(ftte_ctx *c, const double *sigma)
{
    int rc = check_single(c);
    if (rc) return rc;
    if (!sigma) return fail(c, FTTE_ERR_ARG, "ftte_set_output_sigma: bad argument");
    FTTE_HIP(c, hipSetDevice(c->device));
    return c->point.tables.set_sigma(c->stream, sigma, &c->err);
}

int ftte_get_point_rates(ftte_ctx *c, double *rates)
{
    int rc = check_ready(c, false);
    if (rc) return rc;
    if (!rates) return fail(c, FTTE_ERR_ARG, "ftte_get_point_rates: bad argument");
    if (!c->point.rates.ready(c->ncell)) return fail(c, FTTE_ERR_STATE, "no rates: call ftte_set_zero_rates / ftte_point_sources first");
    FTTE_HIP(c, hipSetDevice(c->device));
    double *planes = nullptr;
    if ((rc = c->point.rates.planes(c->stream, &planes, &c->err))) return rc;
    FTTE_HIP(c, hipMemcpyAsync(rates, planes, sizeof(double) * 6 * c->ncell, hipMemcpyDeviceToHost, c->stream));
    FTTE_HIP(c, hipStreamSynchronize(c->stream));
    return FTTE_OK;
}

int ftte_set_point_rates(ftte_ctx *c, const double *rates)
{
    int rc = check_ready(c, false);
    if (rc) return rc;
    if (!rates) return fail(c, FTTE_ERR_ARG, "ftte_set_point_rates: bad argument");
    FTTE_HIP(c, hipSetDevice(c->device));
    return c->point.rates.set(c->stream, c->ncell, rates, &c->err);
}

int ftte_point_rates_device(ftte_ctx *c, double **rates_dev)
{
    int rc = check_ready(c, false);
    if (rc) return rc;
    if (!rates_dev) return fail(c, FTTE_ERR_ARG, "ftte_point_rates_device: bad argument");
    if (!c->point.rates.ready(c->ncell)) return fail(c, FTTE_ERR_STATE, "no rates: call ftte_set_zero_rates / ftte_point_sources first");
    FTTE_HIP(c, hipSetDevice(c->device));
    if ((rc = c->point.rates.planes(c->stream, rates_dev, &c->err))) return rc;
    FTTE_HIP(c, hipStreamSynchronize(c->stream));
    return FTTE_OK;
}

long long ftte_point_ray_steps(const ftte_ctx *c) { return c ? c->point.escape.ray_steps() : 0; }

int ftte_rmax(double *rmax30)
{
    if (!rmax30) return FTTE_ERR_ARG;
    rmax_table(rmax30);
    return FTTE_OK;
}

int ftte_uvb_beta_table(int nfreq, double freqdel, const double *alpha, double *beta, double *ksi, double *gamma)
{
    if (nfreq < 2 || !(freqdel > 0.0) || !alpha || !beta || !ksi || !gamma) return FTTE_ERR_ARG;
    uvb_beta_table(nfreq, freqdel, alpha, beta, ksi, gamma);
    return FTTE_OK;
}

int ftte_coll_rates(double T, int recombination_type, double *k)
{
    if (!(T > 0.0) || (recombination_type != 1 && recombination_type != 2) || !k) return FTTE_ERR_ARG;
    coll_rates(T, recombination_type, k);
    return FTTE_OK;
}

int ftte_rate_coefficient_tables(int nratec, double temstart, double temend, int recombination_type, double *k, double *logtem0,
                                 double *logtem9, double *dlogtem)
{
    if (nratec < 2 || !(temstart > 0.0) || !(temend > temstart) || (recombination_type != 1 && recombination_type != 2) || !k || !logtem0 ||
        !logtem9 || !dlogtem)
        return FTTE_ERR_ARG;
    rate_coefficient_tables(nratec, temstart, temend, recombination_type, k, logtem0, logtem9, dlogtem);
    return FTTE_OK;
}

int ftte_cooling_coefficient_tables(int nratec, double temstart, double temend, int recombination_type, const double *mellema,
                                    const double *gnedin, double *c, double *compa)
{
    if (nratec < 2 || !(temstart > 0.0) || !(temend > temstart) || (recombination_type != 1 && recombination_type != 2) || !c || !compa)
        return FTTE_ERR_ARG;
    if (recombination_type == 2 && (!mellema || !gnedin)) return FTTE_ERR_ARG; // case B interpolates the caller's two arrays
    cooling_coefficient_tables(nratec, temstart, temend, recombination_type, mellema, gnedin, c, compa);
    return FTTE_OK;
}

int ftte_uniform_table(int nfreq, double freqdel, double alpha_quasar, double alpha_stellar, double *ksi, double *gamma)
{
    if (nfreq < 2 || !(freqdel > 0.0) || !ksi || !gamma) return FTTE_ERR_ARG;
    uniform_table(nfreq, freqdel, alpha_quasar, alpha_stellar, ksi, gamma);
    return FTTE_OK;
}

double ftte_dust_cross_section(double lambda_micron, const double *a_smc)
{
    return dust_cross_section(lambda_micron, a_smc);
}

} // extern "C"
