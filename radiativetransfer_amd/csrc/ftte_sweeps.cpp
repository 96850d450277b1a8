// ftte_sweeps.cpp -- the launch sequences of the diffuse sweep: per-direction segment forests on refined cell arrays
// (forest_sweep and its pieces, also used by the hybrid sweep) and cell-fixed bricks on uniform grids (brick_sweep).
#include "ftte_context.h"

namespace ftte {

int ensure_kappa(ftte_ctx *c, int nnu)
{
    const size_t need = (size_t)nnu * c->ncell;
    // the emissivity or source function holds the groups it was set for: with another number of groups the sweep is the plain one,
    // whether the buffers have to grow or not
    if (nnu != c->nnu) c->emit_mode = 0;
    if (c->kappa.source() && c->kappa.capacity() >= need) return FTTE_OK;
    c->emis.release(); c->emit_mode = 0; // sized by the old number of groups: has to be set again
    FTTE_HIP(c, c->kappa.reserve_source(need));
    return FTTE_OK;
}

int ensure_timing(ftte_ctx *c, size_t count)
{
    while (c->timing.size() < count) {
        LaunchTiming t;
        FTTE_HIP(c, t.start.create());
        FTTE_HIP(c, t.stop.create());
        c->timing.push_back(std::move(t));
    }
    return FTTE_OK;
}

// Layout l of a field (or, bricks: its brick-order copy for axis order l, tchunk layers per piece) current on `stream`
static int make_layout(ftte_ctx *c, MediumField &f, int l, hipStream_t stream, bool bricks = false, int tchunk = 0)
{
    if (l == 0 && !bricks) return FTTE_OK; // the source itself
    const MediumField::Copy x = bricks ? MediumField::bricks(l) : MediumField::layout(l);
    if (f.current(x, tchunk)) return FTTE_OK;
    FTTE_HIP(c, f.reserve(x));
    if (launch_to_layout(l, f.source(), f.copy(x), c->n, c->nnu, (long)c->ncell, stream, bricks, tchunk))
        return fail(c, FTTE_ERR_NO_DEVICE, "layout kernel launch failed");
    f.made(x, tchunk);
    return FTTE_OK;
}

int make_cell_major(ftte_ctx *c, MediumField &f, hipStream_t stream, const int32_t *cells, int64_t ncells, long long list)
{
    const size_t count = list ? (size_t)std::max<int64_t>(ncells, 1) : (size_t)c->ncell;
    FTTE_HIP(c, f.reserve(MediumField::kCellMajor, (size_t)c->nnu * count));
    if (f.current(MediumField::kCellMajor, list)) return FTTE_OK;
    if (launch_cell_major(f.source(), f.copy(MediumField::kCellMajor), (long)c->ncell, c->nnu, stream, cells, (long)ncells))
        return fail(c, FTTE_ERR_NO_DEVICE, "layout kernel launch failed");
    f.made(MediumField::kCellMajor, list);
    return FTTE_OK;
}

void fill_brick_group(BrickGroup &G, const BrickPlan &P, size_t g, const double *kappa, const double *emis, double *J, const LayerRec *layers,
                      double *faces, size_t face_stride)
{
    const BrickPlan::Group &H = P.groups[g];
    const DirPlan &D0 = P.dirs[H.dirs[0]];
    G.kappa = kappa; G.emis = emis; G.J = J;
    G.org = D0.org; G.si = D0.si; G.sv = D0.sv; G.su = D0.su;
    G.ndir = (int)H.dirs.size();
    for (size_t q = 0; q < H.dirs.size(); ++q) {
        const int d = H.dirs[q];
        G.dir[q].layers = layers + P.dirs[d].layer_off;
        G.dir[q].faces = faces + (size_t)d * face_stride;
        G.dir[q].w = P.dirs[d].w;
    }
}

int check_ready(ftte_ctx *c, bool need_kappa)
{
    if (c && c->multi)
        return fail(c, FTTE_ERR_UNSUPPORTED, "a multi-device context (ftte_create with ndev > 1) takes host arrays through ftte_set_grid, ftte_set_opacity, "
                                             "ftte_set_emissivity / ftte_set_source_function, ftte_diffuse_sweep and ftte_diffuse_iteration; for "
                                             "everything else create a context per device");
    if (!c) return FTTE_ERR_ARG;
    if (!c->grid_set) return fail(c, FTTE_ERR_STATE, "ftte_set_grid has not been called");
    if (need_kappa && (!c->nnu || !c->kappa.source())) return fail(c, FTTE_ERR_STATE, "no opacities: call ftte_set_opacity / ftte_set_species first");
    return FTTE_OK;
}

// the previous sweep may have been issued on a stream of the caller's: wait for its end before its inputs are rewritten
int wait_sweep(ftte_ctx *c)
{
    if (!c->sweep_pending) return FTTE_OK;
    FTTE_HIP(c, hipEventSynchronize(c->ev_sweep_done));
    c->sweep_pending = false;
    if (const char *why = c->bflow.check_after_sweep(c->bplan.qload)) return fail(c, FTTE_ERR_STALLED, why);
    return FTTE_OK;
}

// The XCC ids this device's workgroups report (HW_REG_XCC_ID), numbered 0 .. count - 1 in ascending order: the persistent form of
// the brick sweep keeps a task queue per XCD.  Once per context.
int xcc_census(ftte_ctx *c)
{
    if (c->xcc_count >= 0) return FTTE_OK;
    DeviceBuffer<unsigned> mask_dev;
    unsigned mask = 0;
    FTTE_HIP(c, mask_dev.reserve(1));
    FTTE_HIP(c, hipMemset(mask_dev, 0, sizeof(unsigned)));
    if (launch_xcc_census(mask_dev, c->stream)) { return fail(c, FTTE_ERR_NO_DEVICE, "census kernel launch failed"); }
    FTTE_HIP(c, hipStreamSynchronize(c->stream));
    FTTE_HIP(c, hipMemcpy(&mask, mask_dev, sizeof(unsigned), hipMemcpyDeviceToHost));
    c->xcc_count = 0;
    for (int x = 0; x < 16; ++x) c->xcc_queue[x] = (mask >> x) & 1u ? (int8_t)c->xcc_count++ : (int8_t)-1;
    return FTTE_OK;
}

int mark_sweep(ftte_ctx *c, hipStream_t stream)
{
    FTTE_HIP(c, c->ev_sweep_done.create(hipEventDisableTiming));
    FTTE_HIP(c, hipEventRecord(c->ev_sweep_done, stream));
    c->sweep_pending = true;
    return FTTE_OK;
}

size_t accumulator_size(DeviceBuffer<double> (&acc)[3][kMaxAcc], size_t per_acc)
{
    size_t have = 0;
    for (auto &layout : acc)
        for (auto &a : layout) have = std::max(have, a.capacity());
    if (have >= per_acc) return have;
    for (auto &layout : acc)
        for (auto &a : layout) a.reset();
    return per_acc;
}

// Tables of several independent runs (`sets`: direction lists that may run side by side on different streams, set q using the
// scratch slots from slot0[q] on), `batch` directions at a time each; built and uploaded in one go on `stream`.  A direction's
// forest may come in passes (hybrid sweep with several boxes): every batch gets per-depth tables pass by pass, and per pass the
// range of the rays that leave its boxes.
int prepare_forests(ftte_ctx *c, hipStream_t stream, const std::vector<std::vector<ForestDir>> &sets, const std::vector<int> &slot0,
                    int batch, size_t per_dir, std::vector<ForestRun> *runs)
{
    std::vector<AmrDirRec> recs;
    std::vector<int64_t> tables;
    runs->assign(sets.size(), ForestRun());
    for (size_t q = 0; q < sets.size(); ++q) {
        const std::vector<ForestDir> &dirs = sets[q];
        ForestRun &R = (*runs)[q];
        const int ndir = (int)dirs.size();
        R.dir_at = recs.size();
        for (int d0 = 0; d0 < ndir; d0 += batch) {
            const int nb = std::min(batch, ndir - d0);
            ForestRun::Batch B;
            B.d0 = d0; B.nb = nb;
            size_t npass = 1;
            for (int t = 0; t < nb; ++t) {
                const ForestTables &D = *dirs[(size_t)(d0 + t)].tables;
                AmrDirRec rec;
                std::memset(&rec, 0, sizeof rec);
                rec.rec = D.rec; rec.active = D.active; rec.w = D.w;
                rec.Iout = c->fscratch.Iout + per_dir * (size_t)(slot0[q] + t);
                rec.mean = c->fscratch.mean + per_dir * (size_t)(slot0[q] + t);
                rec.faces = dirs[(size_t)(d0 + t)].faces; rec.exports = D.exports; rec.nexports = D.nexports;
                rec.imports = D.imports; rec.nimports = D.nimports;
                recs.push_back(rec);
                if (!D.pass_first.empty()) npass = std::max(npass, D.pass_first.size() - 1);
            }
            for (size_t p = 0; p < npass; ++p) {
                ForestRun::Pass P;
                // depth d of pass p is entry first(p) + d of the direction's depth_off, while that lies inside the pass
                auto range = [&](const ForestTables &D, size_t *first, size_t *count) {
                    const size_t all = D.depth_off.size() - 1;
                    if (D.pass_first.empty()) { *first = 0; *count = p == 0 ? all : 0; return; }
                    if (p + 1 >= D.pass_first.size()) { *first = all; *count = 0; return; }
                    *first = (size_t)D.pass_first[p]; *count = (size_t)(D.pass_first[p + 1] - D.pass_first[p]);
                };
                for (int t = 0; t < nb; ++t) {
                    size_t first, count;
                    range(*dirs[(size_t)(d0 + t)].tables, &first, &count);
                    P.maxdepth = std::max(P.maxdepth, count);
                }
                P.table_at = tables.size();
                P.most_at = R.most_of.size();
                for (size_t depth = 0; depth < P.maxdepth; ++depth) {
                    int64_t most = 0;
                    const size_t at = tables.size();
                    tables.resize(at + 2 * (size_t)nb, 0);
                    for (int t = 0; t < nb; ++t) {
                        const ForestTables &D = *dirs[(size_t)(d0 + t)].tables;
                        size_t first, count;
                        range(D, &first, &count);
                        if (depth < count) {
                            const std::vector<int64_t> &off = D.depth_off;
                            tables[at + (size_t)t] = off[first + depth + 1] - off[first + depth];
                            tables[at + (size_t)nb + (size_t)t] = off[first + depth];
                            most = std::max(most, off[first + depth + 1] - off[first + depth]);
                        }
                    }
                    R.most_of.push_back(most);
                }
                // the rays that leave this pass's boxes: count[], first[] per direction
                P.export_at = tables.size();
                tables.resize(P.export_at + 2 * (size_t)nb, 0);
                for (int t = 0; t < nb; ++t) {
                    const ForestTables &D = *dirs[(size_t)(d0 + t)].tables;
                    int64_t first = 0, count = p == 0 ? D.nexports : 0;
                    if (!D.export_first.empty()) {
                        first = p + 1 < D.export_first.size() ? D.export_first[p] : D.nexports;
                        count = p + 1 < D.export_first.size() ? D.export_first[p + 1] - first : 0;
                    }
                    tables[P.export_at + (size_t)t] = count;
                    tables[P.export_at + (size_t)nb + (size_t)t] = first;
                    P.most_exports = std::max(P.most_exports, count);
                }
                B.passes.push_back(P);
            }
            R.batches.push_back(B);
        }
    }
    FTTE_HIP(c, c->fscratch.dirs.reserve(recs.size()));
    FTTE_HIP(c, c->fscratch.tables.reserve(tables.size()));
    if (!recs.empty()) FTTE_HIP(c, hipMemcpyAsync(c->fscratch.dirs, recs.data(), sizeof(AmrDirRec) * recs.size(), hipMemcpyHostToDevice, stream));
    if (!tables.empty()) FTTE_HIP(c, hipMemcpyAsync(c->fscratch.tables, tables.data(), sizeof(int64_t) * tables.size(), hipMemcpyHostToDevice, stream));
    FTTE_HIP(c, hipStreamSynchronize(stream)); // the host vectors leave scope; pageable copies are staged anyway
    return FTTE_OK;
}

// One pass of one batch of a prepared run on `stream`: depth after depth (one launch per depth for the whole batch), then the rays
// that leave the pass's boxes (hybrid sweep) into the bricks' face buffers.
int launch_forest_pass(ftte_ctx *c, hipStream_t stream, const ForestRun &R, size_t b, size_t p, AmrLevelRec A)
{
    const ForestRun::Batch &B = R.batches[b];
    if (p >= B.passes.size()) return FTTE_OK;
    const ForestRun::Pass &P = B.passes[p];
    A.dir = c->fscratch.dirs + R.dir_at + (size_t)B.d0;
    A.ndir = B.nb;
    // Runs of thin levels (option "forest_fuse": at most that many (segment, frequency group) pairs in the fullest direction) go in
    // one launch, a workgroup per direction and a barrier per level; a thick level gets a launch of its own, a thread per pair.
    const int64_t thin = (int64_t)c->opt.launch.forest_fuse;
    for (size_t depth = 0; depth < P.maxdepth;) {
        size_t end = depth;
        while (end < P.maxdepth && R.most_of[P.most_at + end] * (int64_t)c->nnu <= thin) ++end;
        if (end > depth + 1) {
            A.count = A.begin = nullptr; A.most = 0;
            if (launch_amr_levels(A, c->fscratch.tables + P.table_at + depth * 2 * (size_t)B.nb, (int)(end - depth), stream))
                return fail(c, FTTE_ERR_NO_DEVICE, "forest level kernel launch failed");
            depth = end;
            continue;
        }
        A.count = c->fscratch.tables + P.table_at + depth * 2 * (size_t)B.nb;
        A.begin = A.count + B.nb;
        A.most = R.most_of[P.most_at + depth];
        if (launch_amr_level(A, stream)) return fail(c, FTTE_ERR_NO_DEVICE, "forest level kernel launch failed");
        ++depth;
    }
    A.count = c->fscratch.tables + P.export_at;
    A.begin = A.count + B.nb;
    if (launch_amr_export(A, P.most_exports, stream)) return fail(c, FTTE_ERR_NO_DEVICE, "forest export kernel launch failed");
    return FTTE_OK;
}

// The per-leaf means of one batch into J, directions in list order.
int launch_forest_combine(ftte_ctx *c, hipStream_t stream, const ForestRun &R, size_t b, AmrLevelRec A, double *J_dev, bool zero_first)
{
    const ForestRun::Batch &B = R.batches[b];
    A.dir = c->fscratch.dirs + R.dir_at + (size_t)B.d0;
    A.ndir = B.nb;
    if (launch_amr_combine(A, J_dev, zero_first, stream)) return fail(c, FTTE_ERR_NO_DEVICE, "forest combine kernel launch failed");
    return FTTE_OK;
}

// A prepared run on `stream`, batch after batch: its passes, then the means into J.  The combine launches read-modify-write J:
// `before_combine` (if any) is waited for in front of the first one, `after_combine` (if any) recorded behind the last, which is
// how two runs on two streams keep a fixed order of additions.
int launch_forests(ftte_ctx *c, hipStream_t stream, const ForestRun &R, AmrLevelRec A, double *J_dev, bool zero_first, bool time_batches,
                   hipEvent_t before_combine, hipEvent_t after_combine)
{
    const int nnu = c->nnu;
    int rc;
    for (size_t b = 0; b < R.batches.size(); ++b) {
        const ForestRun::Batch &B = R.batches[b];
        if (time_batches) {
            c->timing[b].updates = (int64_t)B.nb * c->ncell * nnu; c->timing[b].lanes = 0;
            FTTE_HIP(c, hipEventRecord(c->timing[b].start, stream));
        }
        for (size_t p = 0; p < B.passes.size(); ++p)
            if ((rc = launch_forest_pass(c, stream, R, b, p, A))) return rc;
        if (b == 0 && before_combine) FTTE_HIP(c, hipStreamWaitEvent(stream, before_combine, 0));
        if ((rc = launch_forest_combine(c, stream, R, b, A, J_dev, zero_first && b == 0))) return rc;
        if (time_batches) {
            FTTE_HIP(c, hipEventRecord(c->timing[b].stop, stream));
            c->timing_used = (int)b + 1;
        }
    }
    if (after_combine) FTTE_HIP(c, hipEventRecord(after_combine, stream));
    return FTTE_OK;
}

// The forests of `dirs`, `batch` directions at a time (A.dir / A.count / A.begin are filled here).
int run_forests(ftte_ctx *c, hipStream_t stream, const std::vector<ForestDir> &dirs, int batch, size_t per_dir, AmrLevelRec A,
                double *J_dev, bool zero_first, bool time_batches)
{
    std::vector<ForestRun> runs;
    int rc;
    if ((rc = prepare_forests(c, stream, {dirs}, {0}, batch, per_dir, &runs))) return rc;
    return launch_forests(c, stream, runs[0], A, J_dev, zero_first, time_batches, nullptr, nullptr);
}

// The sweep on a refined cell array: per-direction segment forests (ftte_amr.h), processed depth by depth.
int forest_sweep(ftte_ctx *c, int ndir, const double *phi, const double *theta, const double *w, const double *uvb,
                 double *J_dev, hipStream_t stream)
{
    const int nnu = c->nnu;
    const int64_t ncell = c->ncell, nseg = 3 * ncell;
    int rc;
    if ((rc = wait_sweep(c))) return rc;

    // ---- plan: fold, link, order; cached while the direction list, the tree and the box stay the same
    std::vector<double> key;
    key.reserve(3 * (size_t)ndir + 1);
    key.push_back(c->box);
    key.insert(key.end(), phi, phi + ndir);
    key.insert(key.end(), theta, theta + ndir);
    key.insert(key.end(), w, w + ndir);
    if (!c->forests.current(key, ndir)) {
        FTTE_HIP(c, hipStreamSynchronize(stream));
        c->forests.drop();
        ++c->n_forest_builds;
        std::vector<double> fphi(ndir), ftheta(ndir);
        std::vector<int> fzone(ndir);
        for (int d = 0; d < ndir; ++d) {
            const int frc = fold_direction(phi[d], theta[d], &fphi[d], &ftheta[d], &fzone[d]);
            if (frc) {
                char buf[160];
                std::snprintf(buf, sizeof buf, "direction %d (phi=%.17g, theta=%.17g) cannot be folded", d, phi[d], theta[d]);
                return fail(c, fold_status(frc), buf);
            }
        }
        c->forests.dirs.resize(ndir);
        // link on the host, a few directions at a time on separate threads, upload, drop the host copy
        const int nthreads = std::max(1u, std::min(16u, std::thread::hardware_concurrency()));
        for (int d0 = 0; d0 < ndir; d0 += nthreads) {
            const int nb = std::min(nthreads, ndir - d0);
            std::vector<AmrForest> F(nb);
            std::vector<std::vector<SegRec>> rec(nb);
            std::vector<std::vector<uint8_t>> active(nb);
            std::vector<int> st(nb, 0);
            std::vector<std::string> msg(nb);
            std::vector<std::thread> pool;
            for (int t = 0; t < nb; ++t)
                pool.emplace_back([&, t] {
                    st[t] = build_forest(c->tree, fphi[d0 + t], ftheta[d0 + t], fzone[d0 + t], c->box, &F[t], &msg[t]);
                    if (st[t]) return;
                    const AmrForest &f = F[t];
                    rec[t] = pack_segments(f);
                    active[t].resize((size_t)ncell);
                    for (int64_t q = 0; q < ncell; ++q)
                        active[t][q] = (uint8_t)((f.up[3 * q + 1] != AmrForest::kInactive ? 1 : 0) | (f.up[3 * q + 2] != AmrForest::kInactive ? 2 : 0));
                });
            for (auto &th : pool) th.join();
            for (int t = 0; t < nb; ++t) {
                if (st[t]) { c->forests.drop(); return fail(c, st[t], "direction " + std::to_string(d0 + t) + ": " + msg[t]); }
                ForestTables &D = c->forests.dirs[d0 + t];
                D.w = w[d0 + t];
                D.depth_off = F[t].depth_off;
                FTTE_HIP(c, to_device(D.rec, rec[t]));
                FTTE_HIP(c, to_device(D.active, active[t]));
            }
        }
        c->forests.key = key;
    }

    // Scratch: outgoing intensity and mean of every segment of every direction of a batch.  The batch is as large as the
    // direction list, kAmrBatch and the free memory allow (two arrays of 3 ncell nnu doubles per direction: 38 GB for 48
    // directions of a 128^3 x 8 tree), and shrinks once more if the allocation still fails.
    const size_t per_dir = (size_t)nseg * nnu;
    const int most = c->opt.hybrid.forest_batch > 0 ? c->opt.hybrid.forest_batch : kAmrBatch;
    if (!c->fscratch.fits(per_dir, ndir, most)) FTTE_HIP(c, hipStreamSynchronize(stream));
    hipError_t why;
    const int batch = c->fscratch.reserve_batch(per_dir, ndir, most, 0.9, true, &why);
    if (!batch) return fail(c, FTTE_ERR_MEMORY, "refined-grid sweep: not enough device memory for the segment scratch of one direction");
    FTTE_HIP(c, hipStreamSynchronize(stream)); // d_uvb below may still be read by the previous sweep
    FTTE_HIP(c, c->d_uvb.send(uvb, (size_t)nnu));

    // the forest path gathers by cell: all groups of a cell side by side (beyond 96 groups the transposing kernel's
    // tile no longer fits the LDS of a workgroup; the strided layout is read as it is)
    const bool cell_major = nnu <= 96;
    if (cell_major && (rc = make_cell_major(c, c->kappa, stream))) return rc;
    if (cell_major && c->emit_mode && (rc = make_cell_major(c, c->emis, stream))) return rc;

    if ((rc = ensure_timing(c, (size_t)((ndir + batch - 1) / batch)))) return rc;
    c->timing_used = 0;
    if (ndir == 0) FTTE_HIP(c, hipMemsetAsync(J_dev, 0, sizeof(double) * (size_t)nnu * ncell, stream));

    {
        AmrLevelRec A;
        std::memset(&A, 0, sizeof A);
        A.kappa = cell_major ? c->kappa.copy(MediumField::kCellMajor) : c->kappa.source();
        A.emis = !c->emit_mode ? nullptr : cell_major ? c->emis.copy(MediumField::kCellMajor) : c->emis.source();
        A.group_stride = cell_major ? 1 : ncell;
        A.cell_stride = cell_major ? nnu : 1;
        A.emit = c->emit_mode;
        A.uvb = c->d_uvb;
        A.ncell = ncell;
        A.nnu = nnu;
        A.math = kMath;
        std::vector<ForestDir> dirs((size_t)ndir);
        for (int d = 0; d < ndir; ++d) dirs[(size_t)d] = ForestDir{&c->forests.dirs[(size_t)d], nullptr};
        if ((rc = run_forests(c, stream, dirs, batch, per_dir, A, J_dev, true, true))) return rc;
    }
    return mark_sweep(c, stream);
}


namespace {

// The brick sweep of a uniform grid, step by step, and what its steps share
struct BrickSweep {
    ftte_ctx *c; const BrickPlan &P; double *J_dev; hipStream_t stream; const HostPipe *pipe; // (what brick_sweep was called with)
    const int n = c->n, nnu = c->nnu;
    const LaunchOptions &O = c->opt.launch;
    // Host arrays (ftte_diffuse_iteration): lanes of frequency groups do their own layouts before their first stage and their own
    // merge after their last.  (With device-resident opacities, layouts up front and one merge at the end are faster: 37.4-38.0
    // against 38.6 ms per 256^3 x 8 x 96 step.  With host arrays in flight the lanes are staggered by the transfers and their ends
    // fall into each other's sweeps anyway.)
    bool lane_ends = false, lane_layout[3] = {false, false, false};
    // Brick order for the opacities and the accumulators (BrickLaunch::tiled, option "tiled": no gain).  For
    // grids made of whole bricks, device-resident opacities, the forms of the kernel that know it; a copy more per axis order.
    bool tiled = false; int tchunk = 0; // tchunk (option 2): a whole brick in one piece
    // Layout 1 ([jc][ic][kc]) holds the rows of layout 0 ([ic][jc][kc]) in another order: its groups march along jc through the
    // layout-0 frame itself (BrickGroup si = +-n, sv = +-n^2), read the source array and leave their accumulators in layout-0 order.  Only
    // layout 2, whose march runs along the contiguous axis, needs a transposed copy.  (Brick order keeps its own copy per layout.)
    int frame[3] = {0, 0, 2};
    // The stage sequence is issued once per "lane" (a subset of the frequency groups, which never touch each other's data, or of the
    // groups of directions) on streams of their own: the tail of one lane's stage overlaps the next stage of another.  Lane 0 is the caller's stream.
    int nulanes = 1, nlanes = 1;
    bool overlap = false; // J merged block by block behind the stages (option "merge_overlap")
    size_t npoints = 0;
    hipStream_t queue(int lane) const { return lane == 0 ? stream : c->lane_stream[(size_t)lane - 1].get(); }
    LaneSlice slice(int lane) const { return lane_slice(nnu, P.glanes > 1 ? 0 : lane, nulanes, c->ncell); }
    BrickLaunch launch(size_t task0, size_t task1, int nu0, int nu1) const
    {
        BrickLaunch L = brick_launch(P, c->btables, task0, task1, nu0, nu1, c->ncell, P.face_elems, c->d_uvb, c->emit_mode);
        L.tiled = tiled ? 1 : 0; L.ablate = O.ablate; L.atomic_acc = O.atomic_acc; L.deal = O.nu_deal;
        return L;
    }
    int prepare(int ndir, const double *uvb), one_launch(), lane_stages(int lane, LaunchTiming &T), merge();
};

// Brick order: cell (brick tu, tv; row r; lane; layer i) of a group at org + i * si + tu * bu + tv * bv + r * sv + lane (63 - lane
// mirrored); tchunk: layer i = tchunk * ti + il + 1 at org + i * si + ti * bi, si = +-piece inside the brick
void tiled_strides(BrickGroup &G, const DirPlan &D0, int n, int tchunk)
{
    const int64_t ntu = n / 64, ntv = n / kBrickRows, piece = 64 * kBrickRows;
    G.sv = D0.sv > 0 ? 64 : -64;
    G.bu = (int32_t)(D0.su > 0 ? piece : -piece);
    G.bv = (int32_t)(D0.sv > 0 ? ntu * piece : -ntu * piece);
    G.org = (int64_t)(D0.si > 0 ? -1 : n) * n * n + (D0.sv > 0 ? 0 : (ntv - 1) * ntu * piece + (kBrickRows - 1) * 64) + (D0.su > 0 ? 0 : (ntu - 1) * piece);
    if (!tchunk) return;
    const int64_t nti = n / tchunk, brick = piece * tchunk;
    G.si = (int32_t)(D0.si > 0 ? piece : -piece);
    G.bu = (int32_t)(D0.su > 0 ? brick : -brick);
    G.bv = (int32_t)(D0.sv > 0 ? ntu * brick : -ntu * brick);
    const int64_t step_i = D0.si > 0 ? ntv * ntu * brick : -ntv * ntu * brick;
    G.bi = step_i - (int64_t)tchunk * G.si;
    // i = 1 (ti = 0, il = 0): the first layer of brick 0 (si > 0) or the last layer of the last brick (si < 0)
    G.org = (D0.si > 0 ? -piece : (nti - 1) * ntv * ntu * brick + (int64_t)tchunk * piece) + (D0.sv > 0 ? 0 : (ntv - 1) * ntu * brick + (kBrickRows - 1) * 64) +
            (D0.su > 0 ? 0 : (ntu - 1) * brick);
}

// Preparation: accumulators and the medium in the layouts the groups march through, the plan's tables, the group records, the
// background, the lanes' streams and events
int BrickSweep::prepare(int ndir, const double *uvb)
{
    int rc;
    const size_t acc_size = accumulator_size(c->acc, (size_t)nnu * c->ncell);
    FTTE_HIP(c, c->d_faces.reserve((size_t)ndir * nnu * (size_t)P.face_elems));
    FTTE_HIP(c, c->merge_stream.create(hipStreamNonBlocking));
    FTTE_HIP(c, c->ev_layout_done.create(hipEventDisableTiming));
    FTTE_HIP(c, c->ev_merge_done.create(hipEventDisableTiming));
    FTTE_HIP(c, c->ev_layouts_ready.create(hipEventDisableTiming));
    lane_ends = pipe != nullptr;
    tiled = O.tiled && !pipe && !c->emit_mode && n % 64 == 0 && n % kBrickRows == 0 && (O.tiled == 1 || n % P.chunk == 0);
    tchunk = tiled && O.tiled == 2 ? P.chunk : 0;
    frame[1] = tiled ? 1 : 0;
    for (int l = 0; l < 3; ++l) {
        for (int s = 0; s < P.nacc[l]; ++s)
            FTTE_HIP(c, c->acc[l][s].reserve(acc_size));
        if (!P.nacc[l] || frame[l] != l) continue;
        if (!lane_ends) {
            if ((rc = make_layout(c, c->kappa, l, stream, tiled, tchunk))) return rc;
        } else if (l) { // (nothing is current: the lanes bring the source) every lane transposes its own groups (lane_stages)
            FTTE_HIP(c, c->kappa.reserve(MediumField::layout(l)));
            lane_layout[l] = true;
        }
        if (c->emit_mode && (rc = make_layout(c, c->emis, l, stream))) return rc;
    }
    FTTE_HIP(c, c->btables.upload(P));
    // the group records carry pointers that depend on nnu (face blocks) and on the buffers: rebuilt per sweep (a few KB)
    std::vector<BrickGroup> G(P.groups.size());
    std::memset(G.data(), 0, sizeof(BrickGroup) * G.size());
    for (size_t g = 0; g < P.groups.size(); ++g) {
        const BrickPlan::Group &H = P.groups[g];
        const DirPlan &D0 = P.dirs[H.dirs[0]];
        const int f = frame[H.layout];
        fill_brick_group(G[g], P, g, tiled ? c->kappa.copy(MediumField::bricks(H.layout)) : c->kappa.in_layout(f), c->emit_mode ? c->emis.in_layout(f) : nullptr,
                         c->acc[H.layout][H.acc], c->btables.layers, c->d_faces, (size_t)nnu * (size_t)P.face_elems);
        if (f != H.layout) { // march (jc) stride n, rows (ic) n^2 apart; a mirrored axis enters from its far end
            const int64_t nn = (int64_t)n * n;
            G[g].si = D0.si > 0 ? n : -n;
            G[g].sv = (int32_t)(D0.sv > 0 ? nn : -nn);
            G[g].org = -1 + (D0.sv > 0 ? -nn : n * nn) + (D0.si > 0 ? -(int64_t)n : nn);
        }
        if (tiled) tiled_strides(G[g], D0, n, tchunk);
    }
    FTTE_HIP(c, c->btables.groups.send(G.data(), G.size()));
    FTTE_HIP(c, c->d_uvb.send(uvb, (size_t)nnu));

    nulanes = P.glanes > 1 ? 1 : std::max(1, std::min(c->opt.brick.lanes, nnu)); // streams over frequency groups ...
    nlanes = nulanes * P.glanes;                                        // ... or over the groups of directions
    FTTE_HIP(c, ensure_lanes(c->lane_stream, c->lane_done, (size_t)nlanes - 1));
    FTTE_HIP(c, c->ev_fork.create(hipEventDisableTiming));
    // (the plan has merge blocks only for stages on one lane of groups; with host arrays every lane merges its own after its stages)
    overlap = O.merge_overlap && !lane_ends && !P.dataflow && P.glanes == 1 && !P.groups.empty() && !P.merge_stage.empty();
    npoints = overlap ? P.merge_stage.size() : 0;
    FTTE_HIP(c, ensure_events(c->ev_merge_point, (size_t)nlanes * npoints, hipEventDisableTiming));
    if ((rc = ensure_timing(c, 1))) return rc;
    c->timing_used = 0;
    return FTTE_OK;
}

// Every brick of the sweep in one launch (options "dataflow" 1..3); flags of the sweep's epoch mark the finished ones
int BrickSweep::one_launch()
{
    BrickLaunch L = launch(0, P.tasks.size(), 0, nnu);
    FTTE_HIP(c, c->bflow.prepare(L, c->btables, P.tasks.size() * (size_t)nnu, stream));
    L.through = c->opt.brick.dataflow == 2 ? 1 : 0;
    int persistent = 0;
    if (P.persistent) {
        L.queue = c->btables.queue;
        std::memcpy(L.qoff, P.qoff, sizeof L.qoff); std::memcpy(L.qlen, P.qlen, sizeof L.qlen); std::memcpy(L.xcc_queue, c->xcc_queue, sizeof L.xcc_queue);
        // as many workgroups as the GPU holds (four waves per SIMD; fewer fit when LDS is padded: the rest start late and
        // find the queues empty)
        hipDeviceProp_t prop;
        FTTE_HIP(c, hipGetDeviceProperties(&prop, c->device));
        persistent = (int)std::min<size_t>((size_t)prop.multiProcessorCount * 16, P.queue.size());
    }
    c->last_brick_form = 0; c->last_brick_dataflow = P.persistent ? 3 : c->opt.brick.dataflow == 2 ? 2 : 1; c->last_brick_whole = 0; c->last_brick_duo = 0;
    const int lrc = launch_brick(L, P.max_dirs, O.brick_waves, O.lds_pad, stream, false, persistent);
    if (lrc) return fail(c, lrc == -1 ? FTTE_ERR_ARG : FTTE_ERR_NO_DEVICE, "brick kernel launch failed");
    FTTE_HIP(c, c->bflow.read_back(P, stream));
    return FTTE_OK;
}

// The stages of one lane on its stream; with host arrays in front of them the lane's opacities and their layouts, behind them its
// merge and its J on the way back
int BrickSweep::lane_stages(int lane, LaunchTiming &T)
{
    const size_t nstages = (size_t)P.nstages;
    int rc;
    hipStream_t q = queue(lane);
    if (lane) FTTE_HIP(c, hipStreamWaitEvent(q, c->ev_fork, 0));
    const LaneSlice S = slice(lane);
    const size_t *off = &P.stage_off[(size_t)(P.glanes > 1 ? lane : 0) * (nstages + 1)];
    if (pipe) {
        // this lane's opacities: after the lane before (one transfer at a time has the link to itself), then its layouts
        FTTE_HIP(c, ensure_events(c->pipe_up, (size_t)nlanes, hipEventDisableTiming));
        if (lane) FTTE_HIP(c, hipStreamWaitEvent(q, c->pipe_up[(size_t)lane - 1], 0));
        if ((rc = upload_on(c, q, c->kappa.source() + S.first, pipe->kappa + S.first, S.bytes))) return rc;
        FTTE_HIP(c, hipEventRecord(c->pipe_up[(size_t)lane], q));
    }
    if (lane_ends) {
        for (int l = 1; l < 3; ++l)
            if (lane_layout[l] && launch_to_layout(l, c->kappa.source() + S.first, c->kappa.in_layout(l) + S.first, n, S.nu1 - S.nu0, (long)c->ncell, q))
                return fail(c, FTTE_ERR_NO_DEVICE, "layout kernel launch failed");
        FTTE_HIP(c, hipEventRecord(T.first[(size_t)lane], q));
    }
    const size_t *seat_off = P.duo ? &P.seat_off[(size_t)(P.glanes > 1 ? lane : 0) * (nstages + 1)] : nullptr;
    for (size_t st = 0, mp = 0; st < nstages; ++st) {
        if (P.duo && seat_off[st + 1] != seat_off[st]) { // two passes per visit: the stage's seats, two wavefronts each
            BrickLaunch L = launch(off[st], off[st + 1], S.nu0, S.nu1);
            L.seats = c->btables.seats + seat_off[st]; L.ntasks = (int)(seat_off[st + 1] - seat_off[st]);
            c->last_brick_form = 0; c->last_brick_dataflow = 0; c->last_brick_whole = 1; c->last_brick_duo = P.nlinked;
            const int lrc = launch_brick(L, P.max_dirs, O.brick_waves, O.lds_pad, q); // (seats: launch_brick_duo)
            if (lrc) return fail(c, lrc == -1 ? FTTE_ERR_ARG : FTTE_ERR_NO_DEVICE, "brick kernel launch failed");
        } else if (!P.duo && off[st + 1] != off[st]) {
            c->last_brick_duo = 0;
            const BrickLaunch L = launch(off[st], off[st + 1], S.nu0, S.nu1);
            const int form = c->opt.brick.brick_form(nnu, c->emit_mode);
            c->last_brick_form = form; c->last_brick_dataflow = 0; c->last_brick_whole = form != 2 && brick_whole_form(L, O.brick_waves);
            const int lrc = form == 2 ? launch_brick_pair(L, P.max_dirs, O.pair_waves, O.lds_pad, q) : launch_brick(L, P.max_dirs, O.brick_waves, O.lds_pad, q);
            if (lrc) return fail(c, lrc == -1 ? FTTE_ERR_ARG : FTTE_ERR_NO_DEVICE, "brick kernel launch failed");
        }
        // (after the stage: this lane's part of the blocks merge point mp waits for, recorded even behind an empty stage)
        if (overlap && mp < npoints && (size_t)P.merge_stage[mp] == st) {
            FTTE_HIP(c, hipEventRecord(c->ev_merge_point[(size_t)lane * npoints + mp], q));
            ++mp;
        }
    }
    if (lane_ends) { // this lane's J: merged as soon as its stages are done, and on its way back (pinned arrays) behind that
        FTTE_HIP(c, hipEventRecord(T.last[(size_t)lane], q));
        const AccList A = acc_list(c->acc, P.nacc, frame, S.first);
        if (launch_merge(A.acc, A.layout, A.count, J_dev + S.first, n, S.nu1 - S.nu0, (long)c->ncell, false, q, nullptr, 0, tiled, tchunk))
            return fail(c, FTTE_ERR_NO_DEVICE, "merge kernel launch failed");
        if (pipe && is_registered(c, pipe->J + S.first, S.bytes))
            FTTE_HIP(c, hipMemcpyAsync(pipe->J + S.first, J_dev + S.first, S.bytes, hipMemcpyDeviceToHost, q));
    }
    if (lane) {
        FTTE_HIP(c, hipEventRecord(c->lane_done[(size_t)lane - 1], q));
        FTTE_HIP(c, hipStreamWaitEvent(stream, c->lane_done[(size_t)lane - 1], 0));
    }
    return FTTE_OK;
}

// J = the groups' accumulators, layout after layout
int BrickSweep::merge()
{
    if (overlap) {
        // block by block as the stages finish them: merge point after merge point, each lane's frequency groups behind that lane's
        // stage; the caller's stream goes on once the last blocks are in
        for (size_t mp = 0; mp < npoints; ++mp)
            for (int lane = 0; lane < nlanes; ++lane) {
                const LaneSlice S = slice(lane);
                const AccList A = acc_list(c->acc, P.nacc, frame, S.first);
                FTTE_HIP(c, hipStreamWaitEvent(c->merge_stream, c->ev_merge_point[(size_t)lane * npoints + mp], 0));
                if (launch_merge_blocks(A.acc, A.layout, A.count, J_dev + S.first, n, S.nu1 - S.nu0, (long)c->ncell, c->btables.merge_blocks + P.merge_off[mp],
                                        (int)(P.merge_off[mp + 1] - P.merge_off[mp]), P.nmb, c->merge_stream, tiled, tchunk))
                    return fail(c, FTTE_ERR_NO_DEVICE, "merge kernel launch failed");
            }
        FTTE_HIP(c, hipEventRecord(c->ev_merge_done, c->merge_stream));
        FTTE_HIP(c, hipStreamWaitEvent(stream, c->ev_merge_done, 0));
    } else if (!lane_ends || P.groups.empty()) {
        const AccList A = acc_list(c->acc, P.nacc, frame);
        if (A.count) {
            if (launch_merge(A.acc, A.layout, A.count, J_dev, n, nnu, (long)c->ncell, false, stream, nullptr, 0, tiled, tchunk))
                return fail(c, FTTE_ERR_NO_DEVICE, "merge kernel launch failed");
        } else FTTE_HIP(c, hipMemsetAsync(J_dev, 0, sizeof(double) * (size_t)nnu * c->ncell, stream)); // no directions
    }
    return FTTE_OK;
}

} // namespace

int brick_sweep(ftte_ctx *c, int ndir, const double *phi, const double *theta, const double *w, const double *uvb, double *J_dev,
                hipStream_t stream, const HostPipe *pipe)
{
    int rc;
    if ((rc = build_brick_plan(c, ndir, phi, theta, w))) return rc;
    // everything below overwrites device tables the previous sweep may still be reading
    if ((rc = wait_sweep(c))) return rc;
    FTTE_HIP(c, hipStreamSynchronize(stream));
    if (stream != c->stream) FTTE_HIP(c, hipStreamSynchronize(c->stream));

    BrickSweep R{c, c->bplan, J_dev, stream, pipe};
    const BrickPlan &P = R.P;
    if ((rc = R.prepare(ndir, uvb))) return rc;
    if (!P.groups.empty()) {
        // One pair of events brackets the whole phase: with kernels of several streams in flight together the time of a single
        // launch says little.
        LaunchTiming &T = c->timing[0];
        T.updates = P.updates * c->nnu; T.lanes = 0;
        if (R.lane_ends) {
            FTTE_HIP(c, ensure_events(T.first, (size_t)R.nlanes, hipEventDefault));
            FTTE_HIP(c, ensure_events(T.last, (size_t)R.nlanes, hipEventDefault));
        }
        FTTE_HIP(c, hipEventRecord(T.start, stream));
        if (P.dataflow && (rc = R.one_launch())) return rc;
        FTTE_HIP(c, hipEventRecord(c->ev_fork, stream));
        for (int lane = 0; lane < R.nlanes && !P.dataflow; ++lane)
            if ((rc = R.lane_stages(lane, T))) return rc;
        if (pipe) { // pageable J: through the staging blocks, lane after lane (the later lanes are still being swept)
            for (int lane = 0; lane < R.nlanes; ++lane) {
                const LaneSlice S = R.slice(lane);
                if (is_registered(c, pipe->J + S.first, S.bytes)) continue;
                if ((rc = download_on(c, R.queue(lane), pipe->J + S.first, J_dev + S.first, S.bytes))) return rc;
            }
            c->kappa.set(); // every lane has brought its groups
        }
        if (R.lane_ends) {
            for (int l = 1; l < 3; ++l) if (R.lane_layout[l]) c->kappa.made(MediumField::layout(l)); // ... and transposed them
            T.lanes = R.nlanes;
        }
        FTTE_HIP(c, hipEventRecord(T.stop, stream));
        c->timing_used = 1;
    }
    if ((rc = R.merge())) return rc;
    return mark_sweep(c, stream);
}


// The sweep of a uniform grid by ray-following tiles (ftte::sweep_kernel, option "engine" = 1): launches of up to `slots`
// directions of one layout, each layout's accumulators merged into J on a second stream while the next layout is swept.
int tile_sweep(ftte_ctx *c, int ndir, const double *phi, const double *theta, const double *w, const double *uvb, double *J_dev,
               hipStream_t stream)
{
    int rc;
    const int n = c->n, nnu = c->nnu;
    const size_t per_acc = (size_t)nnu * c->ncell;
    // the emission variants of the tiled kernel are built for one shape
    const int rows = c->emit_mode ? 8 : c->opt.tile.rows, stack = c->emit_mode ? 1 : c->opt.tile.stack;
    if ((rc = build_plan(c, rows, stack, ndir, phi, theta, w))) return rc;
    Plan &P = c->plan;

    // everything below overwrites device tables the previous sweep may still be reading
    if ((rc = wait_sweep(c))) return rc;
    FTTE_HIP(c, hipStreamSynchronize(stream));
    if (stream != c->stream) FTTE_HIP(c, hipStreamSynchronize(c->stream));

    if (!c->plan_uploaded) {
        FTTE_HIP(c, to_device(c->d_layers, P.layers));
        FTTE_HIP(c, to_device(c->d_items, P.items));
        c->plan_uploaded = true;
    }
    FTTE_HIP(c, c->d_uvb.send(uvb, (size_t)nnu));

    // accumulators sized for this nnu
    const size_t acc_size = accumulator_size(c->acc, per_acc);
    // a second (non-blocking) stream: the transposed copies of the opacity are made there while the directions that march
    // along storage-i (layout 0, the array as it was handed over) are already being swept, and later the merges run there
    FTTE_HIP(c, c->merge_stream.create(hipStreamNonBlocking));
    FTTE_HIP(c, c->ev_layout_done.create(hipEventDisableTiming));
    FTTE_HIP(c, c->ev_merge_done.create(hipEventDisableTiming));
    FTTE_HIP(c, c->ev_layouts_ready.create(hipEventDisableTiming));
    // everything queued on `stream` so far (and the previous sweep's merges) comes first
    FTTE_HIP(c, hipEventRecord(c->ev_layout_done, stream));
    FTTE_HIP(c, hipStreamWaitEvent(c->merge_stream, c->ev_layout_done, 0));
    for (int l = 0; l < 3; ++l) {
        bool any = false;
        for (int s = 0; s < kMaxSlots; ++s) {
            if (!P.used[l][s]) continue;
            any = true;
            FTTE_HIP(c, c->acc[l][s].reserve(acc_size));
        }
        // opacity in the layout this march axis needs
        if (any && (rc = make_layout(c, c->kappa, l, c->merge_stream))) return rc;
        if (any && c->emit_mode && (rc = make_layout(c, c->emis, l, c->merge_stream))) return rc;
    }
    FTTE_HIP(c, hipEventRecord(c->ev_layouts_ready, c->merge_stream));
    bool layouts_awaited = false;

    // events for the launch records
    if ((rc = ensure_timing(c, P.launches.size()))) return rc;
    c->timing_used = 0;

    bool merged_any = false;
    for (size_t li = 0; li < P.launches.size(); ++li) {
        const LaunchPlan &LP = P.launches[li];
        LaunchRec L;
        std::memset(&L, 0, sizeof L);
        for (size_t s = 0; s < LP.dirs.size(); ++s) {
            const DirPlan &D = P.dirs[LP.dirs[s]];
            DirRec &R = L.dir[s];
            R.layers = c->d_layers + D.layer_off;
            R.kappa = c->kappa.in_layout(LP.layout);
            R.J = c->acc[LP.layout][LP.acc_base + s];
            R.emis = c->emit_mode ? c->emis.in_layout(LP.layout) : nullptr;
            R.org = D.org;
            R.si = D.si; R.sv = D.sv; R.su = D.su;
            R.u_lo = D.u_lo; R.v_lo = D.v_lo;
            R.first = LP.first ? 1 : 0;
            R.w = D.w;
        }
        L.items = c->d_items + LP.item_off;
        L.uvb = c->d_uvb;
        L.group_stride = c->ncell;
        L.n = n;
        L.nitems = LP.nitems;
        L.nnu = nnu;
        L.emit = c->emit_mode;
        L.math = kMath;
        LaunchTiming &T = c->timing[li];
        T.updates = LP.updates * nnu; T.lanes = 0;
        if (LP.layout != 0 && !layouts_awaited) { // the first launch that reads a transposed copy
            FTTE_HIP(c, hipStreamWaitEvent(stream, c->ev_layouts_ready, 0));
            layouts_awaited = true;
        }
        FTTE_HIP(c, hipEventRecord(T.start, stream));
        const int lrc = launch_sweep(L, rows, c->opt.tile.waves, stack, nnu, c->opt.launch.lds_pad, stream);
        if (lrc == -1)
            return fail(c, FTTE_ERR_ARG, "no sweep kernel variant for this rows/stack/waves combination (rows x stack: 4x{1,4,8}, "
                                         "8x{1,2,4}, 16x1; waves 2, 3, 4, 6)");
        if (lrc) return fail(c, FTTE_ERR_NO_DEVICE, "sweep kernel launch failed");
        FTTE_HIP(c, hipEventRecord(T.stop, stream));
        c->timing_used = (int)li + 1;

        // J (+)= the accumulators of this layout, slots in order, layout 0 first -- the same sequence of additions as one
        // merge over all of them -- on the second stream, beside the sweeps that follow: the accumulators that the
        // layout's (short) last launch does not touch as soon as the launch before it is done, the rest after the last one.
        // Only the tail of the last layout's merge has nothing to hide behind.
        const bool last_of_layout = li + 1 == P.launches.size() || P.launches[li + 1].layout != LP.layout;
        const bool before_last = !last_of_layout && (li + 2 == P.launches.size() || P.launches[li + 2].layout != LP.layout);
        int lo = -1, hi = -1; // accumulator range [lo, hi) to merge now
        if (before_last && P.launches[li + 1].acc_base > 0) { lo = 0; hi = P.launches[li + 1].acc_base; }
        if (last_of_layout) { lo = LP.acc_base; hi = kMaxSlots; }
        if (lo >= 0) {
            const double *accs[kMaxSlots];
            int layouts[kMaxSlots], count = 0;
            for (int s = lo; s < hi; ++s)
                if (P.used[LP.layout][s]) { accs[count] = c->acc[LP.layout][s]; layouts[count++] = LP.layout; }
            if (count) {
                FTTE_HIP(c, hipEventRecord(c->ev_layout_done, stream));
                FTTE_HIP(c, hipStreamWaitEvent(c->merge_stream, c->ev_layout_done, 0));
                if (launch_merge(accs, layouts, count, J_dev, n, nnu, (long)c->ncell, merged_any, c->merge_stream))
                    return fail(c, FTTE_ERR_NO_DEVICE, "merge kernel launch failed");
                merged_any = true;
            }
        }
    }
    if (!merged_any) FTTE_HIP(c, hipMemsetAsync(J_dev, 0, sizeof(double) * (size_t)nnu * c->ncell, stream)); // no directions
    FTTE_HIP(c, hipEventRecord(c->ev_merge_done, c->merge_stream));
    FTTE_HIP(c, hipStreamWaitEvent(stream, c->ev_merge_done, 0));
    return mark_sweep(c, stream);
}

} // namespace ftte
