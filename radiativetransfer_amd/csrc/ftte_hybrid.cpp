// ftte_hybrid.cpp -- the hybrid sweep of a refined cell array: bricks outside a box around the refined cells, segment forests inside.
#include "ftte_context.h"

namespace ftte {

// ---- hybrid sweep of a refined cell array -----------------------------------------------------------------------------
// The reference recurses into refined cells wherever they are (transport, transportRoutinesModule.f90:577-586) and walks the
// tree for every upstream link of every cell of every direction.  Most of a cell array is plain base cells; here those are
// swept by the brick kernel, and only a box around the refined cells -- widened by one brick, so that its surface separates
// unrefined base cells, across which a ray is handed over exactly as between two bricks -- by the segment forest.  Per group of
// directions: the bricks that do not lie behind the box, then the forest (rays entering it read from the bricks' face
// buffers, rays leaving it written there), then the bricks behind it.  J of a cell = what the bricks stored for the
// directions in whose box it does not lie + what the forest adds for the others.

// The values of a dense cube of `side`^3 cells (the base cells, a fine block) out of a field in leaf order: gathered through
// leaf_of into dst[0], then transposed into the layouts that have accumulators
static int gather_layouts(ftte_ctx *c, const MediumField &f, const int32_t *leaf_of, const LayoutSet &dst, const int (&nacc)[3], int side,
                          hipStream_t stream)
{
    const long cells = (long)side * side * side;
    if (launch_base_cells(f.source(), leaf_of, dst[0], cells, (long)c->ncell, c->nnu, stream))
        return fail(c, FTTE_ERR_NO_DEVICE, "base-cell kernel launch failed");
    for (int l = 1; l < 3; ++l)
        if (nacc[l] && launch_to_layout(l, dst[0], dst[l], side, c->nnu, cells, stream))
            return fail(c, FTTE_ERR_NO_DEVICE, "layout kernel launch failed");
    return FTTE_OK;
}


// The plan for this direction list, tree and set of options, and its forests, leaf list and fine block on the device: kept while
// the key stays the same.  The planner itself reads no context (plan_hybrid, ftte_planner.cpp); the counters are bumped here.
static int build_hybrid_plan(ftte_ctx *c, int ndir, const double *phi, const double *theta, const double *w)
{
    HybridPlan &H = c->hplan;
    const BrickKey K = c->opt.brick.resolve_hybrid(c->n, c->nnu);
    std::vector<double> key = c->opt.hybrid.plan_key(c->box, K.chunk, K.gmax, K.share, ndir, phi, theta, w);
    if (H.valid && H.key == key) return FTTE_OK;
    c->hdev.drop_plan();
    H = HybridPlan();
    H.key = std::move(key);
    std::string why;
    const int rc = plan_hybrid(HybridInputs{c->n, c->box, &c->tree, c->opt.hybrid, K.chunk, K.gmax, K.share, ndir, phi, theta, w}, H, &why);
    c->n_plan_builds += H.brick_plans_made;
    H.bricks.id = ++c->brick_plans; // (new plans: no BrickTables holds them)
    if (H.brick_plans_made > 1) H.fine.plan.id = ++c->brick_plans;
    if (H.forests_linked) ++c->n_forest_builds;
    hipError_t e = hipSuccess;
    // (a new list: the cell-major copies of the medium made for another one are not current)
    if (!rc && H.worthwhile) e = c->hdev.upload(H, H.bricks.w, ++c->leaf_lists);
    if (rc || e != hipSuccess) {
        c->hdev.drop_plan();
        H = HybridPlan();
        return rc ? fail(c, rc, why) : fail(c, FTTE_ERR_NO_DEVICE, std::string("hybrid plan upload: ") + hipGetErrorString(e));
    }
    return FTTE_OK;
}

// What a sweep of the current plan needs on the device beside the plan itself: the map from base cells to leaves, the dense
// layouts and accumulators of the base grid and of the fine block, the face blocks, the base plan's tables, both plans' group
// records, the background, and the forests' scratch (*batch: how many directions of it are resident at a time).
static int reserve_hybrid_buffers(ftte_ctx *c, int ndir, const double *uvb, int64_t face_elems, size_t per_dir, int *batch)
{
    const HybridPlan &H = c->hplan;
    HybridDevice &V = c->hdev;
    const BrickPlan &P = H.bricks;
    const HybridPlan::Fine &FN = H.fine;
    const int n = c->n, nnu = c->nnu, emit = c->emit_mode;
    const int64_t ncell = c->ncell, nbase = (int64_t)n * n * n;
    // ---- device state that depends on the tree only
    if (!V.leaf_of_base) {
        std::vector<int32_t> map((size_t)nbase);
        for (int64_t b = 0; b < nbase; ++b) map[(size_t)b] = c->tree.leaf[(size_t)b];
        FTTE_HIP(c, to_device(V.leaf_of_base, map));
    }
    const size_t per_base = (size_t)nnu * (size_t)nbase;
    FTTE_HIP(c, V.base_kappa.reserve(per_base));
    if (emit) FTTE_HIP(c, V.base_emis.reserve(per_base));
    const size_t acc_size = accumulator_size(c->acc, (size_t)nnu * (size_t)ncell);
    for (int l = 0; l < 3; ++l)
        for (int s = 0; s < P.nacc[l]; ++s) FTTE_HIP(c, c->acc[l][s].reserve(acc_size));
    const size_t face_need = (size_t)ndir * nnu * (size_t)face_elems;
    FTTE_HIP(c, c->d_faces.reserve(face_need));
    FTTE_HIP(c, c->btables.upload(P)); // (the tables the uniform grid's plan uses: whichever of the two swept last holds them)
    // the group records of a plan: its arrays in the three layouts, its accumulators, its part of every direction's face block
    auto send_groups = [&](const BrickPlan &Q, BrickTables &T, const LayoutSet &kappa, const LayoutSet &emis, DeviceBuffer<double> (&acc)[3][kMaxAcc], double *faces) {
        std::vector<BrickGroup> G(Q.groups.size());
        std::memset(G.data(), 0, sizeof(BrickGroup) * G.size());
        for (size_t g = 0; g < Q.groups.size(); ++g) {
            const BrickPlan::Group &Hg = Q.groups[g];
            fill_brick_group(G[g], Q, g, kappa[Hg.layout], emit ? emis[Hg.layout] : nullptr, acc[Hg.layout][Hg.acc], T.layers, faces, (size_t)nnu * (size_t)face_elems);
        }
        return T.groups.send(G.data(), G.size());
    };
    FTTE_HIP(c, send_groups(P, c->btables, V.base_kappa, V.base_emis, c->acc, c->d_faces));
    if (FN.active) {
        // the fine block's own arrays -- opacities in the three layouts, an accumulator per group -- and its group records
        const BrickPlan &Q = FN.plan;
        const size_t per_fine = (size_t)nnu * (size_t)FN.n * FN.n * FN.n;
        FTTE_HIP(c, V.fine_kappa.reserve(per_fine));
        const size_t fine_acc_size = accumulator_size(V.fine_acc, per_fine);
        for (int l = 0; l < 3; ++l)
            for (int a = 0; a < Q.nacc[l]; ++a) FTTE_HIP(c, V.fine_acc[l][a].reserve(fine_acc_size));
        if (emit) FTTE_HIP(c, V.fine_emis.reserve(per_fine));
        FTTE_HIP(c, send_groups(Q, V.fine_tables, V.fine_kappa, V.fine_emis, V.fine_acc, c->d_faces + (size_t)FN.face_base)); // (its faces: behind the base bricks' rings)
    }
    FTTE_HIP(c, c->d_uvb.send(uvb, (size_t)nnu));

    // forest scratch: as forest_sweep, per_dir elements a direction
    // (numbered by the list, a direction's scratch is small: every direction at once, where the memory is there)
    hipError_t no_scratch;
    *batch = c->fscratch.reserve_batch(per_dir, ndir, c->opt.hybrid.forest_batch > 0 ? c->opt.hybrid.forest_batch : 1024, 0.6, false, &no_scratch);
    if (!*batch) return fail(c, FTTE_ERR_NO_DEVICE, std::string("hybrid sweep: no room for the segment scratch: ") + hipGetErrorString(no_scratch));
    return FTTE_OK;
}

// The launches of one sweep (`issue`), or -- option "graph" -- their replay from a hipGraph captured once: the streams' forks and
// joins become dependencies of the graph, and it is replayed while everything the launches name (`sig`) stays the same.
template <typename Issue> static int issue_or_replay(ftte_ctx *c, hipStream_t stream, const std::vector<uintptr_t> &sig, Issue issue)
{
    HybridDevice &V = c->hdev;
    bool replayed = false;
    if (c->opt.hybrid.graph && V.graph_exec && V.graph_sig == sig) {
        if (hipGraphLaunch(V.graph_exec, stream) == hipSuccess) replayed = true;
        else { (void)hipGetLastError(); V.drop_graph(); }
    }
    if (!replayed && c->opt.hybrid.graph) {
        V.drop_graph();
        if (hipStreamBeginCapture(stream, hipStreamCaptureModeRelaxed) == hipSuccess) {
            const int irc = issue();
            hipGraph_t captured = nullptr;
            hipGraphExec_t exec = nullptr;
            const hipError_t e = hipStreamEndCapture(stream, &captured);
            Graph graph;
            graph.adopt(captured);
            if (irc == FTTE_OK && e == hipSuccess && graph && hipGraphInstantiate(&exec, graph, nullptr, nullptr, 0) == hipSuccess) V.graph_exec.adopt(exec);
            if (V.graph_exec && hipGraphLaunch(V.graph_exec, stream) == hipSuccess) {
                V.graph_sig = sig;
                replayed = true;
            } else {
                (void)hipGetLastError();
                V.drop_graph();
                c->opt.hybrid.graph = 0; // this runtime or this sequence does not capture: launches one by one from now on
            }
        } else { (void)hipGetLastError(); c->opt.hybrid.graph = 0; }
    }
    return replayed ? FTTE_OK : issue();
}

int hybrid_sweep(ftte_ctx *c, int ndir, const double *phi, const double *theta, const double *w, const double *uvb, double *J_dev,
                 hipStream_t stream, bool *done)
{
    *done = false;
    int rc;
    // (decided before any device state is touched: the forest path then builds its own plan and scratch, not both)
    if (c->nnu > 96) return FTTE_OK; // the cell-major copy of kappa is what the level kernel reads here: leave it to the forest path
    if ((rc = wait_sweep(c))) return rc;
    FTTE_HIP(c, hipStreamSynchronize(stream));
    if (stream != c->stream) FTTE_HIP(c, hipStreamSynchronize(c->stream));
    if ((rc = build_hybrid_plan(c, ndir, phi, theta, w))) return rc;
    const HybridPlan &H = c->hplan;
    HybridDevice &V = c->hdev;
    if (!H.worthwhile) return FTTE_OK; // the caller takes the forest path for the whole tree
    const BrickPlan &P = H.bricks;
    const int n = c->n, nnu = c->nnu;
    const int64_t ncell = c->ncell, nbase = (int64_t)n * n * n;

    const int emit = c->emit_mode;
    const HybridPlan::Fine &FN = H.fine;
    // a direction's face block: the base bricks' rings, then (a fine block swept by bricks) the fine bricks' own
    const int64_t face_elems = P.face_elems + (FN.active ? FN.plan.face_elems : 0);
    const size_t per_base = (size_t)nnu * (size_t)nbase;
    const size_t per_dir = (size_t)3 * (size_t)std::max<int64_t>(V.ncells, 1) * nnu; // (segments of the leaves of the plan's list only)
    int batch = 0;
    if ((rc = reserve_hybrid_buffers(c, ndir, uvb, face_elems, per_dir, &batch))) return rc;
    // Several passes keep every direction's scratch from pass to pass, and pipelines whose launch lists go by slot have each their
    // own place for a pass (pass_at[pipeline][pass]): with fewer directions resident than the sweep has, all pipelines' forests
    // would have to go in one run at ONE place, in front of bricks of the other pipelines that feed them or behind bricks that
    // read what they export.  Both are left to the forest path for the whole tree.
    if (batch < ndir && (H.npass > 1 || (H.slots && H.nhalves > 1) || FN.active)) return FTTE_OK; // (a fine block's forests come in two passes)
    // the opacities of the boxes' leaves, cell-major, and their emissivity / source function (new every source iteration)
    if ((rc = make_cell_major(c, c->kappa, stream, V.cells, V.ncells, V.cells_id))) return rc;
    if (emit && (rc = make_cell_major(c, c->emis, stream, V.cells, V.ncells, V.cells_id))) return rc;

    if ((rc = ensure_timing(c, 1))) return rc;
    LaunchTiming &Tm = c->timing[0];
    Tm.updates = (int64_t)ndir * ncell * nnu; Tm.lanes = 0;
    c->timing_used = 0;
    const size_t masked_lists = (size_t)H.nhalves * H.nlist;
    const LaunchOptions &launch = c->opt.launch;
    auto brick_stages = [&](int half, size_t from, size_t to, hipStream_t q) -> int {
      for (size_t l = from; l < to; ++l)
        for (int masked = 0; masked < 2; ++masked) { // the stage's whole bricks, then those a box cuts through
            const size_t *off = &H.stage_off[(masked ? masked_lists : 0) + (size_t)half * H.nlist];
            if (off[l + 1] == off[l]) continue;
            BrickLaunch L = brick_launch(P, c->btables, off[l], off[l + 1], 0, nnu, nbase, face_elems, c->d_uvb, emit);
            L.deal = launch.nu_deal;
            const int lrc = launch_brick(L, P.max_dirs, launch.brick_waves, launch.lds_pad, q, masked != 0);
            if (lrc) return fail(c, lrc == -1 ? FTTE_ERR_ARG : FTTE_ERR_NO_DEVICE, "brick kernel launch failed");
        }
      return FTTE_OK;
    };

    // the fine block's own sweep, pipeline `half`: its rays in from the forest, then its bricks stage by stage
    int64_t most_imports = 0;
    for (const ForestTables &D : V.dirs) most_imports = std::max(most_imports, D.nimports);
    auto fine_sweep = [&](int half, hipStream_t q, const ForestRun &R, AmrLevelRec A) -> int {
        const ForestRun::Batch &B = R.batches[0];
        A.dir = c->fscratch.dirs + R.dir_at + (size_t)B.d0;
        A.ndir = B.nb;
        if (launch_amr_fine_import(A, most_imports, q)) return fail(c, FTTE_ERR_NO_DEVICE, "fine import kernel launch failed");
        const BrickPlan &Q = FN.plan;
        for (int st = 0; st < FN.nstages; ++st) {
            const size_t l = (size_t)half * (size_t)FN.nstages + (size_t)st;
            if (FN.stage_off[l + 1] == FN.stage_off[l]) continue;
            BrickLaunch L = brick_launch(Q, V.fine_tables, FN.stage_off[l], FN.stage_off[l + 1], 0, nnu, (int64_t)FN.n * FN.n * FN.n, face_elems, c->d_uvb, emit);
            L.sub = 1; L.deal = launch.nu_deal;
            const int lrc = launch_brick(L, Q.max_dirs, launch.brick_waves, launch.lds_pad, q, false);
            if (lrc) return fail(c, lrc == -1 ? FTTE_ERR_ARG : FTTE_ERR_NO_DEVICE, "brick kernel launch failed");
        }
        return FTTE_OK;
    };

    // ---- per half: bricks not behind the boxes, the forests of the boxes (all directions of the half per depth launch), the
    // bricks behind them.  The halves run side by side on two streams and meet only in J: the second half's means are added
    // after the first half's (an event), the bricks' accumulators after both.
    const int nh = (H.nhalves > 1 && batch >= ndir) ? H.nhalves : 1; // scratch for every direction at once, or one pipeline
    hipStream_t qs[kMaxPipes] = {stream, stream, stream, stream};
    if (nh > 1) {
        FTTE_HIP(c, ensure_lanes(c->lane_stream, c->lane_done, (size_t)nh - 1));
        FTTE_HIP(c, c->ev_fork.create(hipEventDisableTiming));
        for (int r = 0; r < nh; ++r) {
            FTTE_HIP(c, V.ev_combine[r].create(hipEventDisableTiming));
            if (r) qs[r] = c->lane_stream[(size_t)r - 1];
        }
    }
    AmrLevelRec A;
    std::memset(&A, 0, sizeof A);
    A.kappa = c->kappa.copy(MediumField::kCellMajor); A.emis = emit ? c->emis.copy(MediumField::kCellMajor) : nullptr;
    A.group_stride = 1; A.cell_stride = nnu;
    A.emit = emit;
    A.uvb = c->d_uvb;
    A.ncell = ncell; A.nnu = nnu;
    A.cells = V.cells; A.ncells = V.ncells;
    A.face_stride = face_elems;
    A.math = kMath;
    std::vector<ForestRun> runs;
    {
        std::vector<std::vector<ForestDir>> sets((size_t)nh);
        std::vector<int> slot0((size_t)nh, 0);
        for (int h = 0; h < H.nhalves; ++h) {
            const int to = nh > 1 ? h : 0;
            for (int d : H.half_dirs[(size_t)h]) sets[(size_t)to].push_back(ForestDir{&V.dirs[(size_t)d], c->d_faces + (size_t)d * nnu * (size_t)face_elems});
        }
        for (int r = 1; r < nh; ++r) slot0[(size_t)r] = slot0[(size_t)r - 1] + (int)sets[(size_t)r - 1].size();
        // one batch per pipeline when they run side by side (their scratch must not overlap), else `batch` directions at a time
        if ((rc = prepare_forests(c, stream, sets, slot0, nh > 1 ? ndir : batch, per_dir, &runs))) return rc;
    }
    // (FTTE_HYBRID_TIMELINE: events at the phase boundaries of every pipeline, printed when the sweep is over -- a timeline without
    // a tracer, whose own cost per launch changes what overlaps what)
    static const bool timeline = std::getenv("FTTE_HYBRID_TIMELINE") != nullptr;
    struct Mark { Event e; int pipe; const char *what; };
    std::vector<Mark> marks;
    auto mark = [&](hipStream_t q, int pipe, const char *what) {
        if (!timeline) return;
        Event e;
        if (e.create() != hipSuccess) return;
        (void)hipEventRecord(e, q);
        marks.push_back({std::move(e), pipe, what});
    };
    // ---- the launches of one sweep: the same sequence every iteration while plan and buffers stay what they are
    auto issue = [&]() -> int {
        // ---- opacity and emissivity / source function of the base cells in the three layouts, then (a fine block) of its cells,
        // dense in its own storage order; accumulators and J start from zero
        if ((rc = gather_layouts(c, c->kappa, V.leaf_of_base, V.base_kappa, P.nacc, n, stream))) return rc;
        if (emit && (rc = gather_layouts(c, c->emis, V.leaf_of_base, V.base_emis, P.nacc, n, stream))) return rc;
        if (FN.active && (rc = gather_layouts(c, c->kappa, V.leaf_of_fine, V.fine_kappa, FN.plan.nacc, FN.n, stream))) return rc;
        if (FN.active && emit && (rc = gather_layouts(c, c->emis, V.leaf_of_fine, V.fine_emis, FN.plan.nacc, FN.n, stream))) return rc;
        for (int l = 0; l < 3; ++l)
            for (int s = 0; s < P.nacc[l]; ++s) FTTE_HIP(c, hipMemsetAsync(c->acc[l][s], 0, sizeof(double) * per_base, stream));
        FTTE_HIP(c, hipMemsetAsync(J_dev, 0, sizeof(double) * (size_t)nnu * ncell, stream));

        mark(stream, -1, "layouts and zeroing done");
        if (nh > 1) {
            FTTE_HIP(c, hipEventRecord(c->ev_fork, stream));
            for (int r = 1; r < nh; ++r) FTTE_HIP(c, hipStreamWaitEvent(qs[r], c->ev_fork, 0));
        }
        // Issued list by list, alternating between the streams, so that none waits for the host to finish with the others.  In
        // front of list pass_at[k] of a pipeline its forests of pass k; behind the last pass the means into J.
        for (size_t l = 0; l <= H.nlist; ++l) {
            for (int h = 0; h < H.nhalves; ++h) {
                const int r = nh > 1 ? h : 0;
                for (int pass = 0; pass < H.npass; ++pass) {
                    if ((size_t)H.pass_at[(size_t)h][(size_t)pass] != l || (nh == 1 && h > 0)) continue;
                    hipEvent_t before = (nh > 1 && r > 0) ? V.ev_combine[r - 1].get() : nullptr, after = (nh > 1 && r + 1 < nh) ? V.ev_combine[r].get() : nullptr;
                    if (FN.active) { // the forest before the fine block's bricks, those, the forest behind them; the means below
                        mark(qs[r], r, "bricks before the box done");
                        if ((rc = launch_forest_pass(c, qs[r], runs[(size_t)r], 0, 0, A))) return rc;
                        mark(qs[r], r, "forest before the fine block done");
                        if ((rc = fine_sweep(h, qs[r], runs[(size_t)r], A))) return rc;
                        mark(qs[r], r, "fine bricks done");
                        if ((rc = launch_forest_pass(c, qs[r], runs[(size_t)r], 0, 1, A))) return rc;
                        mark(qs[r], r, "forest behind the fine block done");
                        continue;
                    }
                    mark(qs[r], r, "bricks before a forest pass done");
                    if (H.npass == 1) { // one pass: batch by batch, each with its means
                        if ((rc = launch_forests(c, qs[r], runs[(size_t)r], A, J_dev, false, false, before, after))) return rc;
                        continue;
                    }
                    // (several passes: every direction of the run is resident, one batch)
                    if ((rc = launch_forest_pass(c, qs[r], runs[(size_t)r], 0, (size_t)pass, A))) return rc;
                }
                if (l < H.nlist && (rc = brick_stages(h, l, l + 1, qs[r]))) return rc;
            }
        }
        // several passes: the means into J when everything is issued, pipeline after pipeline (a pipeline's last pass may come
        // earlier or later than another's, and the events that order the additions must be recorded before they are waited for)
        for (int r = 0; r < nh; ++r) mark(qs[r], r, "last bricks done");
        if (H.npass > 1 || FN.active)
            for (int r = 0; r < nh; ++r) {
                if (nh > 1 && r > 0) FTTE_HIP(c, hipStreamWaitEvent(qs[r], V.ev_combine[r - 1], 0));
                if ((rc = launch_forest_combine(c, qs[r], runs[(size_t)r], 0, A, J_dev, false))) return rc;
                if (nh > 1 && r + 1 < nh) FTTE_HIP(c, hipEventRecord(V.ev_combine[r], qs[r]));
            }
        for (int r = 1; r < nh; ++r) {
            FTTE_HIP(c, hipEventRecord(c->lane_done[(size_t)r - 1], qs[r]));
            FTTE_HIP(c, hipStreamWaitEvent(stream, c->lane_done[(size_t)r - 1], 0));
        }

        // ---- J of the unrefined base cells += what the bricks stored (layout after layout, accumulator after accumulator)
        {
            const AccList B = acc_list(c->acc, P.nacc, kOwnFrame);
            if (B.count && launch_merge(B.acc, B.layout, B.count, J_dev, n, nnu, (long)nbase, true, stream, V.leaf_of_base, (long)ncell))
                return fail(c, FTTE_ERR_NO_DEVICE, "merge kernel launch failed");
        }
        if (FN.active) { // ... and J of the fine block's cells += what its bricks stored
            const AccList B = acc_list(V.fine_acc, FN.plan.nacc, kOwnFrame);
            if (B.count && launch_merge(B.acc, B.layout, B.count, J_dev, FN.n, nnu, (long)FN.n * FN.n * FN.n, true, stream, V.leaf_of_fine, (long)ncell))
                return fail(c, FTTE_ERR_NO_DEVICE, "merge kernel launch failed");
        }
        return FTTE_OK;
    };

    // The sequence is hundreds of short launches on up to three streams (more with several passes).  Option "graph" = 1 captures it
    // once into a hipGraph -- the streams' forks and joins become dependencies of the graph -- and replays it while the plan, J and
    // every buffer and table the launches name stay the same.  Measured on ROCm 7.2 / MI355X the replay is SLOWER than issuing the
    // launches (configs[3]: 15.8 against 12.2 ms; 8 clusters in 5 passes: 23.9 against 15.1 ms), so it is off by default.
    // What the captured launches name: every owner appends the addresses and parameters it holds, the sweep its own.  (No entry
    // for the LDS pad or the other options: every accepted option but "nu_deal" invalidates the plan, and a rebuilt plan drops the
    // captured graph.)
    std::vector<uintptr_t> sig = {(uintptr_t)J_dev, (uintptr_t)stream, (uintptr_t)nnu, (uintptr_t)nh, (uintptr_t)launch.brick_waves, (uintptr_t)emit, (uintptr_t)launch.forest_fuse,
                                  (uintptr_t)c->d_faces.get(), (uintptr_t)c->d_uvb.get()};
    V.sign(sig, FN.active, FN.plan.nacc);
    c->fscratch.sign(sig);
    c->kappa.sign(sig); c->emis.sign(sig);
    sign_tables(c->btables, sig);
    for (int l = 0; l < 3; ++l) for (int s2 = 0; s2 < P.nacc[l]; ++s2) sig.push_back((uintptr_t)c->acc[l][s2].get());
    FTTE_HIP(c, hipEventRecord(Tm.start, stream));
    if ((rc = issue_or_replay(c, stream, sig, issue))) return rc;
    FTTE_HIP(c, hipEventRecord(Tm.stop, stream));
    if (timeline && !marks.empty()) {
        (void)hipEventSynchronize(Tm.stop);
        for (const Mark &m : marks) {
            float ms = 0.f;
            (void)hipEventElapsedTime(&ms, Tm.start, m.e);
            std::fprintf(stderr, "[ftte] hybrid timeline: %8.3f ms  pipeline %2d  %s\n", ms, m.pipe, m.what);
        }
        float ms = 0.f;
        (void)hipEventElapsedTime(&ms, Tm.start, Tm.stop);
        std::fprintf(stderr, "[ftte] hybrid timeline: %8.3f ms  sweep done (means and merges in)\n", ms);
    }
    c->timing_used = 1;
    *done = true;
    return mark_sweep(c, stream);
}


} // namespace ftte
