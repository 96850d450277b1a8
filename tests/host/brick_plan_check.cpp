// The uniform grid's planners (radiativetransfer_amd/csrc/ftte_planner.cpp: plan_bricks, plan_tiles) and the rules that turn the
// brick options into a plan's parameters (ftte_bricks.h: BrickOptions) against a stub of the HIP runtime (tests/host/stub), under
// the address and undefined-behaviour sanitizers.  Direction sets: all 48 pixels of HEALPix nside 2 (groups of 1, 2 and 3
// directions), all 192 of nside 4 (72 groups of 2 and 3, stage offsets up to 3 and 6) and one direction per izone.  Every plan is
// checked for what it must hold -- every (group, brick) once, in the list of its stage and lane, the groups with the most directions
// first, exactly the first visitor of an accumulator's brick stores, each dependency the right neighbour and earlier in the list, the
// merge points around the blocks' last writers, the queues with whole dependency chains -- and its FNV-1a-64 digests are pinned to
// what build_brick_plan / build_plan produced before they were cut into steps.  `--print` prints the table instead of comparing.
#include <algorithm>
#include <array>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "ftte_geometry.h"
#include "ftte_tiles.h"

using namespace ftte;

static const char *g_case = "";
#define CHECK(cond)                                                                                                \
    do {                                                                                                           \
        if (!(cond)) { std::fprintf(stderr, "ERROR %s:%d (%s): %s\n", __FILE__, __LINE__, g_case, #cond); std::exit(1); } \
    } while (0)

static uint64_t fnv(uint64_t h, const void *p, size_t bytes)
{
    const unsigned char *b = (const unsigned char *)p;
    for (size_t i = 0; i < bytes; ++i) { h ^= b[i]; h *= 1099511628211ull; }
    return h;
}
constexpr uint64_t kSeed = 14695981039346656037ull;
template <typename T> static uint64_t fnv_ints(uint64_t h, const std::vector<T> &v) // as 64-bit integers, whatever the host's types
{
    for (const T &x : v) { const int64_t y = (int64_t)x; h = fnv(h, &y, 8); }
    return h;
}

struct Dirs { std::vector<double> phi, theta, w; int ndir() const { return (int)phi.size(); } };
static Dirs healpix(int nside) // every pixel
{
    Dirs D;
    const int64_t npix = 12 * (int64_t)nside * nside;
    for (int64_t ipix = 0; ipix < npix; ++ipix) {
        double p, t;
        CHECK(pix2ang_nest(nside, ipix, &p, &t) == 0);
        D.phi.push_back(p); D.theta.push_back(t); D.w.push_back(1.0 / (double)npix);
    }
    return D;
}
static Dirs one_per_izone() // the first pixel of each izone at nside 4
{
    const Dirs all = healpix(4);
    Dirs D;
    D.phi.assign(24, 0); D.theta.assign(24, 0); D.w.assign(24, 1.0 / 24);
    bool have[25] = {};
    for (int d = 0; d < all.ndir(); ++d) {
        double fp, ft;
        int izone = 0;
        CHECK(fold_direction(all.phi[(size_t)d], all.theta[(size_t)d], &fp, &ft, &izone) == 0 && izone >= 1 && izone <= 24);
        if (!have[izone]) { have[izone] = true; D.phi[(size_t)izone - 1] = all.phi[(size_t)d]; D.theta[(size_t)izone - 1] = all.theta[(size_t)d]; }
    }
    for (int z = 1; z <= 24; ++z) CHECK(have[z]);
    return D;
}

static BrickOptions options(int chunk, int group, int share, int team, int lanes, int dataflow, int queue_mix)
{
    BrickOptions o;
    o.chunk = chunk; o.group = group; o.share = share; o.team = team; o.lanes = lanes; o.dataflow = dataflow; o.queue_mix = queue_mix;
    return o;
}
// what the cached caller does with the options: resolve, settle the persistent form with the XCD count, plan
static BrickKey key_of(const BrickOptions &opt, int n, int nnu, int emit_mode, int xcc_count)
{
    BrickKey key = opt.resolve(n, nnu, emit_mode);
    key.box = 1.0;
    if (key.want_dataflow && opt.dataflow == 3) opt.persistent(key, nnu, xcc_count);
    return key;
}

// ---- a brick plan: what it must hold ---------------------------------------------------------------------------------------------
struct TaskAt { int g, tu, tv, ti, lane, stage; bool accumulates; };

static size_t physical_brick(const BrickPlan &P, const BrickPlan::Group &G, int tu, int tv, int ti)
{
    const DirPlan &D0 = P.dirs[(size_t)G.dirs[0]];
    const int bu = D0.su < 0 ? P.ntu - 1 - tu : tu, bv = D0.sv < 0 ? P.ntv - 1 - tv : tv, bi = D0.si < 0 ? P.nti - 1 - ti : ti;
    return ((size_t)bi * P.ntv + bv) * P.ntu + bu;
}

static void check_brick_plan(const BrickPlan &P, const BrickKey &key, const Dirs &D, int nnu)
{
    const int n = key.n, ng = (int)P.groups.size(), ns = P.nstages;
    const size_t nb = (size_t)P.ntu * P.ntv * P.nti, nt = P.tasks.size();
    CHECK(P.valid && P.n == n && P.chunk == key.chunk && P.ntu == (n + 63) / 64 && P.ntv == (n + kBrickRows - 1) / kBrickRows && P.nti == (n + key.chunk - 1) / key.chunk);
    CHECK(P.dataflow == (key.want_dataflow != 0) && (int)P.dirs.size() == D.ndir() && P.layers.size() == (size_t)D.ndir() * n);
    // the groups partition the directions, at most gmax each, one izone and layout each
    std::vector<int> seen_dir((size_t)D.ndir(), 0);
    int nacc = 0, max_offset = 0;
    for (const auto &G : P.groups) {
        CHECK(!G.dirs.empty() && (int)G.dirs.size() <= key.gmax && G.lane >= 0 && G.lane < P.glanes && G.acc >= 0 && G.acc < P.nacc[G.layout] && G.offset >= 0);
        for (int d : G.dirs) CHECK(d >= 0 && d < D.ndir() && !seen_dir[(size_t)d]++ && P.dirs[(size_t)d].izone == G.izone && P.dirs[(size_t)d].layout == G.layout);
        max_offset = std::max(max_offset, G.offset);
    }
    for (int d = 0; d < D.ndir(); ++d) CHECK(seen_dir[(size_t)d] == 1);
    for (int l = 0; l < 3; ++l) nacc += P.nacc[l];
    CHECK(P.glanes == std::max(1, std::min(key.want_glanes, nacc)) && ns == P.ntu + P.ntv + P.nti - 2 + max_offset);
    // the groups of one accumulator on one lane
    std::vector<int> lane_of_acc(3 * (size_t)kMaxAcc, -1);
    for (const auto &G : P.groups) {
        int &l = lane_of_acc[(size_t)G.layout * kMaxAcc + G.acc];
        CHECK(l < 0 || l == G.lane);
        l = G.lane;
    }
    // ---- lists: [glanes][nstages + 1], contiguous, covering the tasks; a task in list tu + tv + ti + offset of its group's lane
    CHECK(P.stage_off.size() == (size_t)P.glanes * (size_t)(ns + 1) && P.stage_off[0] == 0 && P.stage_off.back() == nt);
    std::vector<TaskAt> tasks(nt);
    std::vector<int> times(ng * nb, 0);
    for (int l = 0; l < P.glanes; ++l) {
        const size_t *off = &P.stage_off[(size_t)l * (size_t)(ns + 1)];
        if (l > 0) CHECK(off[0] == off[-1]);
        for (int st = 0; st < ns; ++st) {
            CHECK(off[st] <= off[st + 1]);
            for (size_t q = off[st]; q < off[st + 1]; ++q) {
                const BrickTask &T = P.tasks[q];
                TaskAt &A = tasks[q];
                A = TaskAt{T.group, T.tu, T.tv, T.ti & (kBrickAccumulate - 1), l, st, (T.ti & kBrickAccumulate) != 0};
                CHECK(A.g >= 0 && A.g < ng && A.tu >= 0 && A.tu < P.ntu && A.tv >= 0 && A.tv < P.ntv && A.ti < P.nti);
                const BrickPlan::Group &G = P.groups[(size_t)A.g];
                CHECK(G.lane == l && st == A.tu + A.tv + A.ti + G.offset);
                CHECK(times[(size_t)A.g * nb + ((size_t)A.ti * P.ntv + A.tv) * P.ntu + A.tu]++ == 0);
                if (q > off[st]) { // within a list: the groups with the most directions first, then in index order, bricks in storage order
                    const TaskAt &B = tasks[q - 1];
                    const size_t sa = G.dirs.size(), sb = P.groups[(size_t)B.g].dirs.size();
                    CHECK(sb > sa || (sb == sa && (B.g < A.g || (B.g == A.g && std::array<int, 3>{B.ti, B.tv, B.tu} < std::array<int, 3>{A.ti, A.tv, A.tu}))));
                }
            }
        }
    }
    CHECK(nt == ng * nb);
    CHECK(P.updates == (int64_t)n * n * n * D.ndir());
    // ---- per accumulator and physical brick: exactly the visitor in the earliest stage stores, all later ones accumulate; prev[q]:
    // the visitor before q
    std::vector<std::vector<std::pair<int, int32_t>>> visitors(3 * (size_t)kMaxAcc * nb);
    for (size_t q = 0; q < nt; ++q) {
        const BrickPlan::Group &G = P.groups[(size_t)tasks[q].g];
        visitors[((size_t)G.layout * kMaxAcc + G.acc) * nb + physical_brick(P, G, tasks[q].tu, tasks[q].tv, tasks[q].ti)].push_back({tasks[q].stage, (int32_t)q});
    }
    std::vector<int32_t> prev(nt, -1);
    for (auto &V : visitors) {
        std::sort(V.begin(), V.end());
        for (size_t k = 0; k < V.size(); ++k) {
            if (k > 0) { CHECK(V[k].first > V[k - 1].first); prev[(size_t)V[k].second] = V[k - 1].second; } // (never two in one stage)
            CHECK(tasks[(size_t)V[k].second].accumulates == (k > 0));
        }
    }
    // ---- dependencies (one-launch forms)
    if (P.dataflow && nt) {
        CHECK(P.deps.size() == nt * kBrickDeps);
        std::vector<int32_t> index(ng * nb, -1);
        auto at = [&](int g, int tu, int tv, int ti) { return index[(size_t)g * nb + ((size_t)ti * P.ntv + tv) * P.ntu + tu]; };
        for (size_t q = 0; q < nt; ++q) index[(size_t)tasks[q].g * nb + ((size_t)tasks[q].ti * P.ntv + tasks[q].tv) * P.ntu + tasks[q].tu] = (int32_t)q;
        for (size_t q = 0; q < nt; ++q) {
            const TaskAt &A = tasks[q];
            const int32_t *dep = &P.deps[q * kBrickDeps];
            for (int k = 0; k < kBrickDeps; ++k) CHECK(dep[k] >= -1 && dep[k] < (int32_t)q);
            CHECK(dep[0] == (A.tu > 0 ? at(A.g, A.tu - 1, A.tv, A.ti) : -1));
            CHECK(dep[1] == (A.tv > 0 ? at(A.g, A.tu, A.tv - 1, A.ti) : -1));
            CHECK(dep[2] == (A.ti > 0 ? at(A.g, A.tu, A.tv, A.ti - 1) : -1));
            CHECK(dep[3] == prev[q]);
            CHECK(dep[4] == (A.ti >= 2 && A.tu + 1 < P.ntu ? at(A.g, A.tu + 1, A.tv, A.ti - 2) : -1));
            CHECK(dep[5] == (A.ti >= 2 && A.tv + 1 < P.ntv ? at(A.g, A.tu, A.tv + 1, A.ti - 2) : -1));
        }
    } else CHECK(P.deps.empty());
    // ---- merge blocks and merge points (a launch per stage, one lane of groups)
    if (!P.dataflow && P.glanes == 1 && nt) {
        const int nmb = (n + kMergeBlock - 1) / kMergeBlock;
        const size_t nblk = (size_t)nmb * nmb * nmb;
        CHECK(P.nmb == nmb && P.merge_blocks.size() == nblk);
        std::vector<int> last(nblk, -1);
        for (size_t q = 0; q < nt; ++q) {
            const TaskAt &A = tasks[q];
            const BrickPlan::Group &G = P.groups[(size_t)A.g];
            const DirPlan &D0 = P.dirs[(size_t)G.dirs[0]];
            // the brick's cells along the frame axes (march, v, u) and the storage axis each of them is
            const int axis[3] = {G.layout, G.layout == 0 ? 1 : 0, G.layout == 2 ? 1 : 2};
            const int first[3] = {P.chunk * A.ti, kBrickRows * A.tv, 64 * A.tu}, size[3] = {P.chunk, kBrickRows, 64};
            const bool mirror[3] = {D0.si < 0, D0.sv < 0, D0.su < 0};
            int lo[3], hi[3];
            for (int a = 0; a < 3; ++a) {
                const int x0 = first[a], x1 = std::min(n, first[a] + size[a]) - 1;
                lo[axis[a]] = (mirror[a] ? n - 1 - x1 : x0) / kMergeBlock;
                hi[axis[a]] = (mirror[a] ? n - 1 - x0 : x1) / kMergeBlock;
            }
            for (int bi = lo[0]; bi <= hi[0]; ++bi)
                for (int bj = lo[1]; bj <= hi[1]; ++bj)
                    for (int bk = lo[2]; bk <= hi[2]; ++bk) { int &s = last[((size_t)bi * nmb + bj) * nmb + bk]; s = std::max(s, A.stage); }
        }
        std::vector<int> times_block(nblk, 0);
        const size_t np = P.merge_stage.size();
        CHECK(np >= 1 && P.merge_off.size() == np + 1 && P.merge_off[0] == 0 && P.merge_off[np] == nblk && P.merge_stage[np - 1] == ns - 1);
        for (size_t m = 0; m < np; ++m) {
            CHECK(m == 0 || P.merge_stage[m] > P.merge_stage[m - 1]);
            CHECK(P.merge_off[m] <= P.merge_off[m + 1]);
            for (size_t k = P.merge_off[m]; k < P.merge_off[m + 1]; ++k) {
                const int32_t b = P.merge_blocks[k];
                CHECK(b >= 0 && (size_t)b < nblk && times_block[(size_t)b]++ == 0 && last[(size_t)b] >= 0);
                CHECK(last[(size_t)b] <= P.merge_stage[m] && (m == 0 || last[(size_t)b] > P.merge_stage[m - 1]));
            }
        }
    } else CHECK(P.nmb == 0 && P.merge_blocks.empty() && P.merge_stage.empty() && P.merge_off.empty());
    // ---- queues (persistent form): every (task, frequency group) once, what it waits for earlier in its own queue
    CHECK(P.persistent == (key.want_dataflow == 3 && nt > 0));
    if (P.persistent) {
        const int nq = key.xcc_count;
        CHECK(nq >= 1 && nq <= kBrickQueues && P.queue.size() == nt * (size_t)nnu);
        std::vector<int32_t> queue_of(nt * (size_t)nnu, -1);
        std::vector<uint32_t> place(nt * (size_t)nnu, 0);
        int64_t load = 0;
        for (int q = 0; q < kBrickQueues; ++q) {
            CHECK(P.qoff[q] == (q == 0 ? 0 : P.qoff[q - 1] + P.qlen[q - 1]));
            if (q >= nq) CHECK(P.qlen[q] == 0 && P.qload[q] == 0);
            load += P.qload[q];
            for (uint32_t k = P.qoff[q]; k < P.qoff[q] + P.qlen[q]; ++k) {
                const uint32_t id = P.queue[k];
                CHECK(id < nt * (size_t)nnu && queue_of[id] < 0);
                queue_of[id] = q; place[id] = k;
                if (nnu % nq == 0 && key.queue_mix == 0) CHECK(q == (int)(id % (uint32_t)nnu) % nq);
            }
        }
        CHECK(P.qoff[kBrickQueues - 1] + P.qlen[kBrickQueues - 1] == P.queue.size() && load == P.updates * nnu);
        for (size_t id = 0; id < queue_of.size(); ++id) {
            CHECK(queue_of[id] >= 0);
            for (int k = 0; k < kBrickDeps; ++k) {
                const int32_t dep = P.deps[(id / (size_t)nnu) * kBrickDeps + (size_t)k];
                if (dep < 0) continue;
                const size_t dep_id = (size_t)dep * (size_t)nnu + id % (size_t)nnu;
                CHECK(queue_of[dep_id] == queue_of[id] && place[dep_id] < place[id]);
            }
        }
    } else CHECK(P.queue.empty());
}

struct BrickDigests { uint64_t tasks, lists, deps, merge, queues; };
static BrickDigests digests_of(const BrickPlan &P)
{
    BrickDigests G;
    G.tasks = fnv(kSeed, P.tasks.data(), sizeof(BrickTask) * P.tasks.size());
    G.lists = fnv_ints(kSeed, P.stage_off);
    for (const auto &g : P.groups) G.lists = fnv_ints(G.lists, std::vector<int>{g.izone, g.layout, g.acc, g.offset, g.lane, (int)g.dirs.size()});
    G.lists = fnv_ints(G.lists, std::vector<int64_t>{P.nacc[0], P.nacc[1], P.nacc[2], P.vface_off, P.iface_off, P.uqface_off, P.face_elems, P.ut, P.uw, P.nslot, P.max_dirs,
                                                     P.glanes, P.nstages, P.updates});
    G.deps = fnv_ints(kSeed, P.deps);
    G.merge = fnv_ints(fnv_ints(fnv_ints(kSeed, P.merge_blocks), P.merge_stage), P.merge_off);
    G.queues = fnv_ints(kSeed, P.queue);
    for (int q = 0; q < kBrickQueues; ++q) G.queues = fnv_ints(G.queues, std::vector<int64_t>{P.qoff[q], P.qlen[q], P.qload[q]});
    return G;
}

// what a case resolves to and plans, pinned to the planner before it was cut into steps
struct BrickWant { int want_dataflow, chunk, gmax, glanes, nstages, points, nmb; size_t ntasks; BrickDigests d; };

// ---- the tile plan ---------------------------------------------------------------------------------------------------------------
struct TileDigests { uint64_t items, launches, layers; };
struct TileWant { size_t nitems, nlaunches; int short_batches; TileDigests d; };

static TileWant check_tile_plan(const Plan &P, const TileInputs &in)
{
    const int n = in.n;
    CHECK(P.valid && (int)P.dirs.size() == in.ndir && P.layers.size() == (size_t)in.ndir * n);
    std::vector<int> launched((size_t)in.ndir, 0);
    bool used[3][kMaxSlots] = {}, begun[3] = {};
    size_t next = 0;
    int short_batches = 0;
    for (const LaunchPlan &LP : P.launches) {
        CHECK(LP.item_off == next && LP.nitems > 0 && !LP.dirs.empty() && (int)LP.dirs.size() <= in.slots && LP.acc_base >= 0 && LP.acc_base + (int)LP.dirs.size() <= in.slots);
        CHECK(LP.first == !begun[LP.layout] && LP.updates == (int64_t)n * n * n * (int64_t)LP.dirs.size());
        CHECK((LP.acc_base > 0) == (!LP.first && (int)LP.dirs.size() < in.slots)); // (a short last batch takes the highest accumulators)
        begun[LP.layout] = true;
        if (LP.acc_base > 0) ++short_batches;
        for (size_t s = 0; s < LP.dirs.size(); ++s) {
            CHECK(LP.dirs[s] >= 0 && LP.dirs[s] < in.ndir && !launched[(size_t)LP.dirs[s]]++ && P.dirs[(size_t)LP.dirs[s]].layout == LP.layout);
            CHECK(s == 0 || LP.dirs[s] > LP.dirs[s - 1]);
            used[LP.layout][LP.acc_base + (int)s] = true;
        }
        std::vector<std::array<int, 3>> tiles;
        for (int k = 0; k < LP.nitems; ++k) {
            const WorkItem &it = P.items[LP.item_off + (size_t)k];
            CHECK(it.slot >= 0 && it.slot < (int)LP.dirs.size());
            const DirPlan &D = P.dirs[(size_t)LP.dirs[(size_t)it.slot]];
            CHECK(it.tu >= 0 && it.tu < D.ntu && it.tv >= 0 && it.tv < D.ntv && it.i_first >= 1 && it.i_first <= it.i_last && it.i_last <= n && it.pad == 0);
            if (k > 0) { const WorkItem &b = P.items[LP.item_off + (size_t)k - 1]; CHECK(b.i_last - b.i_first >= it.i_last - it.i_first); } // longest marches first
            tiles.push_back({it.slot, it.tu, it.tv});
        }
        std::sort(tiles.begin(), tiles.end());
        CHECK(std::adjacent_find(tiles.begin(), tiles.end()) == tiles.end());
        next += (size_t)LP.nitems;
    }
    CHECK(next == P.items.size());
    for (int d = 0; d < in.ndir; ++d) CHECK(launched[(size_t)d] == 1);
    for (int l = 0; l < 3; ++l) for (int s = 0; s < kMaxSlots; ++s) CHECK(P.used[l][s] == used[l][s]);
    TileWant W;
    W.nitems = P.items.size(); W.nlaunches = P.launches.size(); W.short_batches = short_batches;
    W.d.items = fnv(kSeed, P.items.data(), sizeof(WorkItem) * P.items.size());
    W.d.launches = kSeed;
    for (const LaunchPlan &LP : P.launches) {
        W.d.launches = fnv_ints(W.d.launches, std::vector<int64_t>{LP.layout, LP.first, LP.acc_base, (int64_t)LP.item_off, LP.nitems, LP.updates});
        W.d.launches = fnv_ints(W.d.launches, LP.dirs);
    }
    for (const DirPlan &D : P.dirs) W.d.launches = fnv_ints(W.d.launches, std::vector<int64_t>{D.izone, D.layout, D.org, D.si, D.sv, D.su, D.u_lo, D.v_lo, D.ntu, D.ntv, D.du_mid, D.dv_mid, (int64_t)D.layer_off, D.slot});
    W.d.layers = fnv(kSeed, P.layers.data(), sizeof(LayerRec) * P.layers.size());
    return W;
}

// ---- option resolution -----------------------------------------------------------------------------------------------------------
static void check_options()
{
    g_case = "options";
    auto resolved = [](const BrickOptions &o, int n, int nnu, int emit) { const BrickKey k = o.resolve(n, nnu, emit); return std::array<int, 5>{k.chunk, k.gmax, k.share, k.want_dataflow, k.want_glanes}; };
    auto R = [](int chunk, int gmax, int share, int want_dataflow, int want_glanes) { return std::array<int, 5>{chunk, gmax, share, want_dataflow, want_glanes}; };
    // chunk by the frequency groups, never above the grid; the groups go to the streams where the frequency groups are fewer than the lanes
    CHECK(resolved(BrickOptions(), 64, 1, 0) == R(4, 3, 2, 0, 2));
    CHECK(resolved(BrickOptions(), 64, 2, 0) == R(8, 3, 2, 0, 1));
    CHECK(resolved(BrickOptions(), 64, 3, 0) == R(8, 3, 2, 0, 1));
    CHECK(resolved(BrickOptions(), 64, 4, 0) == R(16, 3, 2, 0, 1));
    CHECK(resolved(BrickOptions(), 64, 8, 0) == R(16, 3, 2, 0, 1));
    CHECK(resolved(BrickOptions(), 5, 8, 0) == R(5, 3, 2, 0, 1));
    // team and emit_mode: the form decides gmax at one frequency group, and switches the one-launch forms off
    for (int emit = 0; emit <= 2; ++emit) {
        CHECK(options(0, 0, 2, -1, 2, 0, 0).brick_form(1, emit) == 2 && options(0, 0, 2, -1, 2, 0, 0).brick_form(4, emit) == 2);
        CHECK(options(0, 0, 2, -1, 2, 0, 0).brick_form(8, emit) == (emit ? 2 : 0) && options(0, 0, 2, -1, 2, 1, 0).brick_form(1, emit) == 0);
        CHECK(options(0, 0, 2, 0, 2, 0, 0).brick_form(1, emit) == 0 && options(0, 0, 2, 2, 2, 1, 0).brick_form(8, emit) == 2);
        CHECK(resolved(options(0, 0, 2, -1, 2, 0, 0), 64, 1, emit) == R(4, 3, 2, 0, 2));
        CHECK(resolved(options(0, 0, 2, 0, 2, 0, 0), 64, 1, emit) == R(4, 2, 2, 0, 2));
        CHECK(resolved(options(0, 0, 2, 2, 2, 0, 0), 64, 1, emit) == R(4, 3, 2, 0, 2));
        CHECK(resolved(options(0, 0, 2, 0, 2, 0, 0), 64, 2, emit) == R(8, 3, 2, 0, 1));
        for (int dataflow = 1; dataflow <= 3; ++dataflow) {
            CHECK(resolved(options(0, 0, 2, -1, 2, dataflow, 0), 64, 1, emit) == R(4, 2, 2, emit ? 0 : 1, emit ? 2 : 1));
            CHECK(resolved(options(0, 0, 2, -1, 2, dataflow, 0), 64, 8, emit) == R(16, 3, 2, emit ? 0 : 1, 1));
            CHECK(resolved(options(0, 0, 2, 0, 2, dataflow, 0), 64, 8, emit) == R(16, 3, 2, emit ? 0 : 1, 1));
            CHECK(resolved(options(0, 0, 2, 2, 2, dataflow, 0), 64, 8, emit) == R(16, 3, 2, 0, 1));
        }
    }
    // one launch needs whole bricks: n a multiple of 64, of the rows and of the chunk
    CHECK(resolved(options(0, 0, 2, -1, 2, 1, 0), 70, 8, 0) == R(16, 3, 2, 0, 1));
    CHECK(resolved(options(0, 0, 2, -1, 2, 1, 0), 128, 8, 0) == R(16, 3, 2, 1, 1));
    CHECK(resolved(options(24, 0, 2, -1, 2, 1, 0), 128, 8, 0) == R(24, 3, 2, 0, 1));
    // lanes against the frequency groups; explicit chunk, group and share
    CHECK(resolved(options(0, 0, 2, -1, 1, 0, 0), 64, 1, 0) == R(4, 3, 2, 0, 1));
    CHECK(resolved(options(0, 0, 2, -1, 4, 0, 0), 64, 1, 0) == R(4, 3, 2, 0, 4));
    CHECK(resolved(options(0, 0, 2, -1, 4, 0, 0), 64, 2, 0) == R(8, 3, 2, 0, 4));
    CHECK(resolved(options(0, 0, 2, -1, 4, 0, 0), 64, 4, 0) == R(16, 3, 2, 0, 1));
    CHECK(resolved(options(0, 0, 2, -1, 4, 1, 0), 64, 2, 0) == R(8, 3, 2, 1, 1));
    CHECK(resolved(options(32, 1, 0, -1, 2, 0, 0), 64, 8, 0) == R(32, 1, 0, 0, 1));
    CHECK(resolved(options(4096, 8, 1, -1, 2, 0, 0), 70, 1, 0) == R(70, 8, 1, 0, 2));
    // the persistent form: only where one launch is possible, option "dataflow" is 3 and the XCDs are 1 .. kBrickQueues
    const BrickKey k3 = key_of(options(0, 0, 2, -1, 2, 3, 1), 64, 6, 0, 8), k1 = key_of(options(0, 0, 2, -1, 2, 1, 1), 64, 6, 0, 8);
    CHECK(k3.want_dataflow == 3 && k3.nnu == 6 && k3.xcc_count == 8 && k3.queue_mix == 1 && k1.want_dataflow == 1 && k1.nnu == 0 && k1.xcc_count == 0 && k1.queue_mix == 0);
    CHECK(!(k3 == k1) && !(k3 == key_of(options(0, 0, 2, -1, 2, 3, 1), 64, 6, 0, 4)) && !(k3 == key_of(options(0, 0, 2, -1, 2, 3, 0), 64, 6, 0, 8)));
    CHECK(k3 == key_of(options(0, 0, 2, -1, 2, 3, 1), 64, 6, 0, 8) && key_of(options(0, 0, 2, -1, 2, 3, 0), 64, 8, 0, 0) == key_of(options(0, 0, 2, -1, 2, 1, 0), 64, 8, 0, 8));
    CHECK(key_of(options(0, 0, 2, -1, 2, 3, 0), 64, 8, 0, kBrickQueues + 1).want_dataflow == 1 && key_of(options(0, 0, 2, -1, 2, 3, 0), 64, 8, 0, kBrickQueues).want_dataflow == 3);
    // partial bricks: options "dataflow" 1 and 3 resolve to the key of 0 (queue_mix and the XCDs do not enter it): no rebuild
    CHECK(key_of(options(0, 0, 2, -1, 2, 0, 0), 70, 8, 0, 8) == key_of(options(0, 0, 2, -1, 2, 1, 0), 70, 8, 0, 8));
    CHECK(key_of(options(0, 0, 2, -1, 2, 0, 0), 70, 8, 0, 8) == key_of(options(0, 0, 2, -1, 2, 3, 2), 70, 8, 0, 4));
    CHECK(!(key_of(options(0, 0, 2, -1, 2, 0, 0), 70, 8, 0, 8) == key_of(options(0, 0, 2, -1, 2, 0, 0), 72, 8, 0, 8)));
    // the hybrid sweep's base plan: short bricks, gmax by the frequency groups alone
    auto hybrid = [](const BrickOptions &o, int n, int nnu) { const BrickKey k = o.resolve_hybrid(n, nnu); return std::array<int, 5>{k.chunk, k.gmax, k.share, k.want_dataflow, k.n}; };
    CHECK(hybrid(BrickOptions(), 64, 1) == R(4, 2, 2, 0, 64) && hybrid(BrickOptions(), 64, 2) == R(4, 3, 2, 0, 64) && hybrid(BrickOptions(), 64, 8) == R(4, 3, 2, 0, 64));
    CHECK(hybrid(options(0, 0, 1, 2, 2, 3, 0), 64, 1) == R(4, 2, 1, 0, 64) && hybrid(options(16, 4, 2, -1, 2, 0, 0), 8, 1) == R(8, 4, 2, 0, 8) && hybrid(BrickOptions(), 3, 1) == R(3, 2, 2, 0, 3));
}

// Expectations, case by case in the order of the tables in main(): what build_brick_plan / build_plan of the commit before the
// planners were cut into steps resolved and planned for the same inputs (this program's `--print`, run against that commit's
// ftte_plan.cpp through a harness that fills a context from the options).
static const BrickWant kBrickWant[] = {
    {0, 4, 3, 2, 2, 0, 0, 48, {0xe74c111e76ff8485ull, 0x4711d9dab3d60975ull, 0xcbf29ce484222325ull, 0xcbf29ce484222325ull, 0xab0c262759a1d225ull}}, // n 5, nnu 1
    {0, 5, 3, 1, 1, 1, 1, 24, {0xaa4b2471267ad325ull, 0xb3083b4d4cacf175ull, 0xcbf29ce484222325ull, 0xed87496f429bab84ull, 0xab0c262759a1d225ull}}, // n 5, nnu 2
    {0, 4, 3, 2, 23, 0, 0, 3072, {0xb9021faed0706525ull, 0x65f089702e461953ull, 0xcbf29ce484222325ull, 0xcbf29ce484222325ull, 0xab0c262759a1d225ull}}, // n 64, nnu 1
    {0, 8, 3, 1, 15, 1, 2, 1536, {0x328b643cc2a00ba5ull, 0xa1e4ce283919cca1ull, 0xcbf29ce484222325ull, 0x9e07f76108c41c43ull, 0xab0c262759a1d225ull}}, // n 64, nnu 2
    {0, 16, 3, 1, 11, 1, 2, 768, {0x72d8f99d96e813a5ull, 0x30cc9f4103a08779ull, 0xcbf29ce484222325ull, 0x38a69c4ffe6bc5c7ull, 0xab0c262759a1d225ull}}, // n 64, nnu 8
    {0, 4, 3, 2, 23, 0, 0, 3072, {0xe4bfb806fccda965ull, 0x5a8b405bc2e8d431ull, 0xcbf29ce484222325ull, 0xcbf29ce484222325ull, 0xab0c262759a1d225ull}}, // n 64, nnu 1, 48 directions
    {0, 8, 3, 1, 15, 1, 2, 1536, {0x43c9c39811ea8e25ull, 0x493963b1a8f94b03ull, 0xcbf29ce484222325ull, 0x9e07f76108c41c43ull, 0xab0c262759a1d225ull}}, // n 64, nnu 2, 48 directions
    {0, 16, 3, 1, 11, 1, 2, 768, {0x8fd646dc32afd825ull, 0x941e7473e1b7cd1bull, 0xcbf29ce484222325ull, 0x38a69c4ffe6bc5c7ull, 0xab0c262759a1d225ull}}, // n 64, nnu 8, 48 directions
    {0, 16, 3, 1, 11, 1, 2, 768, {0x0d7781ff48289a25ull, 0x815d8b623d7aeb97ull, 0xcbf29ce484222325ull, 0x38a69c4ffe6bc5c7ull, 0xab0c262759a1d225ull}}, // n 64, nnu 8, 48 directions, share 0
    {0, 4, 2, 2, 25, 0, 0, 3584, {0xfb6f9494385616e5ull, 0x58673468c58d0719ull, 0xcbf29ce484222325ull, 0xcbf29ce484222325ull, 0xab0c262759a1d225ull}}, // n 64, nnu 1, 48 directions, team 0
    {0, 4, 2, 2, 25, 0, 0, 3584, {0xfb6f9494385616e5ull, 0x58673468c58d0719ull, 0xcbf29ce484222325ull, 0xcbf29ce484222325ull, 0xab0c262759a1d225ull}}, // n 64, nnu 1, 48 directions, emissivity
    {0, 2, 1, 4, 43, 0, 0, 12288, {0x407e3d724f6236c5ull, 0xfd8eadf13960eaa2ull, 0xcbf29ce484222325ull, 0xcbf29ce484222325ull, 0xab0c262759a1d225ull}}, // n 64, nnu 2, 48 directions, chunk 2, group 1, lanes 4
    {0, 16, 3, 1, 14, 2, 2, 2304, {0x3f756a1ab29a9005ull, 0xdcb8f14f1ef1083dull, 0xcbf29ce484222325ull, 0x74a18814035a3048ull, 0xab0c262759a1d225ull}}, // n 64, nnu 8, 192 directions, share 1
    {0, 16, 3, 1, 17, 2, 2, 2304, {0xcc7d86b15b565165ull, 0x1384a518ca2639efull, 0xcbf29ce484222325ull, 0xaa64844430e6d017ull, 0xab0c262759a1d225ull}}, // n 64, nnu 8, 192 directions, share 2
    {0, 16, 3, 1, 14, 2, 3, 2160, {0x72ccd4e0e9a6d8a5ull, 0x4f0650c941dfef76ull, 0xcbf29ce484222325ull, 0xe9a59ac8dc471457ull, 0xab0c262759a1d225ull}}, // n 70, nnu 8, 48 directions
    {0, 16, 3, 1, 14, 2, 3, 2160, {0x72ccd4e0e9a6d8a5ull, 0x4f0650c941dfef76ull, 0xcbf29ce484222325ull, 0xe9a59ac8dc471457ull, 0xab0c262759a1d225ull}}, // n 70, nnu 8, 48 directions, dataflow 1
    {0, 16, 3, 1, 14, 2, 3, 2160, {0x72ccd4e0e9a6d8a5ull, 0x4f0650c941dfef76ull, 0xcbf29ce484222325ull, 0xe9a59ac8dc471457ull, 0xab0c262759a1d225ull}}, // n 70, nnu 8, 48 directions, dataflow 3
    {0, 8, 3, 1, 35, 3, 5, 20808, {0x4979a697ff85d0e5ull, 0x1056b7e7de5bb502ull, 0xcbf29ce484222325ull, 0xfae7650a07a84c0eull, 0xab0c262759a1d225ull}}, // n 130, nnu 2
    {1, 16, 3, 1, 11, 0, 0, 768, {0x8fd646dc32afd825ull, 0xd0fb369ce1dbc4c3ull, 0x7b7fe7ee2d0da8b5ull, 0xcbf29ce484222325ull, 0xab0c262759a1d225ull}}, // n 64, nnu 8, 48 directions, dataflow 1
    {1, 16, 3, 1, 17, 0, 0, 2304, {0xcc7d86b15b565165ull, 0x2c5d764ecc9fc4a7ull, 0xd669f9c0f5d490bdull, 0xcbf29ce484222325ull, 0xab0c262759a1d225ull}}, // n 64, nnu 8, 192 directions, dataflow 1
    {1, 16, 3, 1, 11, 0, 0, 768, {0x0d7781ff48289a25ull, 0x8a87233a76075d4full, 0x579d758ffa654c1dull, 0xcbf29ce484222325ull, 0xab0c262759a1d225ull}}, // n 64, nnu 4, 48 directions, dataflow 2, share 1
    {1, 16, 3, 1, 24, 0, 0, 6144, {0xcde2c0544f48e8a5ull, 0x1ebffcc99ad2f866ull, 0xed1663ab19b132afull, 0xcbf29ce484222325ull, 0xab0c262759a1d225ull}}, // n 128, nnu 8, 48 directions, dataflow 1
    {1, 4, 3, 1, 48, 0, 0, 24576, {0x9ae4eabb92b46fa5ull, 0x8696c40bcb6e1131ull, 0x90310fd874f460eeull, 0xcbf29ce484222325ull, 0xab0c262759a1d225ull}}, // n 128, nnu 2, dataflow 1, chunk 4
    {3, 16, 3, 1, 11, 0, 0, 768, {0x8fd646dc32afd825ull, 0xd0fb369ce1dbc4c3ull, 0x7b7fe7ee2d0da8b5ull, 0xcbf29ce484222325ull, 0x0aaddd2f591e0c4dull}}, // n 64, nnu 8, 48 directions, dataflow 3
    {3, 16, 3, 1, 11, 0, 0, 768, {0x8fd646dc32afd825ull, 0xd0fb369ce1dbc4c3ull, 0x7b7fe7ee2d0da8b5ull, 0xcbf29ce484222325ull, 0xca44a3b040e4a0f1ull}}, // n 64, nnu 6, 48 directions, dataflow 3
    {3, 16, 3, 1, 11, 0, 0, 768, {0x8fd646dc32afd825ull, 0xd0fb369ce1dbc4c3ull, 0x7b7fe7ee2d0da8b5ull, 0xcbf29ce484222325ull, 0x2a17b6cd6314c70dull}}, // n 64, nnu 8, 48 directions, dataflow 3, queue_mix 1
    {3, 16, 3, 1, 11, 0, 0, 768, {0x8fd646dc32afd825ull, 0xd0fb369ce1dbc4c3ull, 0x7b7fe7ee2d0da8b5ull, 0xcbf29ce484222325ull, 0xc4ef30d94b594bedull}}, // n 64, nnu 8, 48 directions, dataflow 3, queue_mix 2
    {3, 16, 3, 1, 24, 0, 0, 6144, {0x1484c03399df0ba5ull, 0x3cc6b107c2cd08cbull, 0xad754ba5a9c8d3e7ull, 0xcbf29ce484222325ull, 0x06547d026ce3b465ull}}, // n 128, nnu 6, dataflow 3, 4 XCDs
    {1, 16, 3, 1, 11, 0, 0, 768, {0x8fd646dc32afd825ull, 0xd0fb369ce1dbc4c3ull, 0x7b7fe7ee2d0da8b5ull, 0xcbf29ce484222325ull, 0xab0c262759a1d225ull}}, // n 64, nnu 8, 48 directions, dataflow 3, no XCD
    {1, 16, 3, 1, 11, 0, 0, 768, {0x8fd646dc32afd825ull, 0xd0fb369ce1dbc4c3ull, 0x7b7fe7ee2d0da8b5ull, 0xcbf29ce484222325ull, 0xab0c262759a1d225ull}}, // n 64, nnu 8, 48 directions, dataflow 3, 9 XCDs
};
static const TileWant kTileWant[] = {
    {1300, 6, 0, {0xaed811734a059af5ull, 0x9cc888c0392219eeull, 0xcb75b40bc5931fe1ull}}, // tiles: n 64, rows 8, stack 1, slots 8
    {122, 6, 0, {0xc3b112ca6864d512ull, 0xd3fca0057fa79c2full, 0x0ce1aa5cec52b08full}}, // tiles: n 5, rows 4, stack 1, slots 8
    {728, 6, 0, {0x68df8b43481e64a5ull, 0x76c612ee34b5903eull, 0xa211541c2b3a2863ull}}, // tiles: n 70, rows 16, stack 1, slots 8
    {728, 12, 3, {0xfd1c996bb6b20745ull, 0xc57fb124bbc79d07ull, 0xa211541c2b3a2863ull}}, // tiles: n 70, rows 8, stack 2, slots 5
    {4332, 12, 3, {0x4b6e4da2510270d4ull, 0x4ae2e57069b0a6bfull, 0xc7a1a26bad232504ull}}, // tiles: n 130, rows 8, stack 1, slots 5
    {4332, 6, 0, {0x5c3a2a333da23665ull, 0xfeffd3856c2338c2ull, 0xc7a1a26bad232504ull}}, // tiles: n 130, rows 4, stack 2, slots 8
    {48, 12, 3, {0x686d1fbddf25c5c1ull, 0x5da1ee1851eb0adaull, 0x0ce1aa5cec52b08full}}, // tiles: n 5, rows 16, stack 2, slots 5
};

int main(int argc, char **argv)
{
    const bool print = argc > 1 && !std::strcmp(argv[1], "--print");
    const Dirs sets[3] = {one_per_izone(), healpix(2), healpix(4)}; // 24, 48, 192 directions
    check_options();

    const BrickOptions def = BrickOptions();
    struct BrickCase { const char *name; int set, n, nnu, emit_mode, xcc_count; BrickOptions opt; };
    const BrickCase bricks[] = {
        // the smallest grid: two stages on two lanes of groups and no merge blocks; one stage and one merge point
        {"n 5, nnu 1", 0, 5, 1, 0, 8, def},
        {"n 5, nnu 2", 0, 5, 2, 0, 8, def},
        // whole bricks, one direction per izone: 23 stages of chunk 4, 15 of chunk 8, 11 of chunk 16 with 2^3 merge blocks
        {"n 64, nnu 1", 0, 64, 1, 0, 8, def},
        {"n 64, nnu 2", 0, 64, 2, 0, 8, def},
        {"n 64, nnu 8", 0, 64, 8, 0, 8, def},
        // groups of 1, 2 and 3 directions: the visiting order differs from the index order
        {"n 64, nnu 1, 48 directions", 1, 64, 1, 0, 8, def},
        {"n 64, nnu 2, 48 directions", 1, 64, 2, 0, 8, def},
        {"n 64, nnu 8, 48 directions", 1, 64, 8, 0, 8, def},
        {"n 64, nnu 8, 48 directions, share 0", 1, 64, 8, 0, 8, options(0, 0, 0, -1, 2, 0, 0)},
        {"n 64, nnu 1, 48 directions, team 0", 1, 64, 1, 0, 8, options(0, 0, 2, 0, 2, 0, 0)},
        {"n 64, nnu 1, 48 directions, emissivity", 1, 64, 1, 1, 8, options(0, 0, 2, -1, 2, 1, 0)},
        {"n 64, nnu 2, 48 directions, chunk 2, group 1, lanes 4", 1, 64, 2, 0, 8, options(2, 1, 2, -1, 4, 0, 0)},
        // 72 groups of 2 and 3: stage offsets up to 3 (share 1) and 6 (share 2), 14 and 17 stages
        {"n 64, nnu 8, 192 directions, share 1", 2, 64, 8, 0, 8, options(0, 0, 1, -1, 2, 0, 0)},
        {"n 64, nnu 8, 192 directions, share 2", 2, 64, 8, 0, 8, def},
        // partial bricks: the one-launch forms fall back; 3^3 merge blocks, two merge points
        {"n 70, nnu 8, 48 directions", 1, 70, 8, 0, 8, def},
        {"n 70, nnu 8, 48 directions, dataflow 1", 1, 70, 8, 0, 8, options(0, 0, 2, -1, 2, 1, 0)},
        {"n 70, nnu 8, 48 directions, dataflow 3", 1, 70, 8, 0, 8, options(0, 0, 2, -1, 2, 3, 0)},
        // 5^3 merge blocks, three merge points, 20808 tasks
        {"n 130, nnu 2", 0, 130, 2, 0, 8, def},
        // one launch: the dependency table
        {"n 64, nnu 8, 48 directions, dataflow 1", 1, 64, 8, 0, 8, options(0, 0, 2, -1, 2, 1, 0)},
        {"n 64, nnu 8, 192 directions, dataflow 1", 2, 64, 8, 0, 8, options(0, 0, 2, -1, 2, 1, 0)},
        {"n 64, nnu 4, 48 directions, dataflow 2, share 1", 1, 64, 4, 0, 8, options(0, 0, 1, -1, 2, 2, 0)},
        {"n 128, nnu 8, 48 directions, dataflow 1", 1, 128, 8, 0, 8, options(0, 0, 2, -1, 2, 1, 0)},
        {"n 128, nnu 2, dataflow 1, chunk 4", 0, 128, 2, 0, 8, options(4, 0, 2, -1, 2, 1, 0)},
        // persistent workgroups: queue = frequency group mod 8; dealt by load; the other mixes; no queues without a usable XCD count
        {"n 64, nnu 8, 48 directions, dataflow 3", 1, 64, 8, 0, 8, options(0, 0, 2, -1, 2, 3, 0)},
        {"n 64, nnu 6, 48 directions, dataflow 3", 1, 64, 6, 0, 8, options(0, 0, 2, -1, 2, 3, 0)},
        {"n 64, nnu 8, 48 directions, dataflow 3, queue_mix 1", 1, 64, 8, 0, 8, options(0, 0, 2, -1, 2, 3, 1)},
        {"n 64, nnu 8, 48 directions, dataflow 3, queue_mix 2", 1, 64, 8, 0, 8, options(0, 0, 2, -1, 2, 3, 2)},
        {"n 128, nnu 6, dataflow 3, 4 XCDs", 0, 128, 6, 0, 4, options(0, 0, 2, -1, 2, 3, 0)},
        {"n 64, nnu 8, 48 directions, dataflow 3, no XCD", 1, 64, 8, 0, 0, options(0, 0, 2, -1, 2, 3, 0)},
        {"n 64, nnu 8, 48 directions, dataflow 3, 9 XCDs", 1, 64, 8, 0, kBrickQueues + 1, options(0, 0, 2, -1, 2, 3, 0)},
    };
    const size_t nbricks = sizeof bricks / sizeof bricks[0];
    CHECK(print || sizeof kBrickWant / sizeof kBrickWant[0] == nbricks);
    for (size_t k = 0; k < nbricks; ++k) {
        const BrickCase &K = bricks[k];
        g_case = K.name;
        const Dirs &D = sets[K.set];
        const BrickKey key = key_of(K.opt, K.n, K.nnu, K.emit_mode, K.xcc_count);
        BrickPlan P;
        std::string why;
        const int rc = plan_bricks(BrickInputs{key, D.ndir(), D.phi.data(), D.theta.data(), D.w.data()}, P, &why);
        if (rc) std::fprintf(stderr, "ERROR %s: plan_bricks: %d %s\n", K.name, rc, why.c_str());
        CHECK(rc == 0);
        check_brick_plan(P, key, D, K.nnu);
        const BrickDigests G = digests_of(P);
        std::printf("    {%d, %d, %d, %d, %d, %d, %d, %zu, {0x%016llxull, 0x%016llxull, 0x%016llxull, 0x%016llxull, 0x%016llxull}}, // %s\n", key.want_dataflow, key.chunk,
                    key.gmax, P.glanes, P.nstages, (int)P.merge_stage.size(), P.nmb, P.tasks.size(), (unsigned long long)G.tasks, (unsigned long long)G.lists,
                    (unsigned long long)G.deps, (unsigned long long)G.merge, (unsigned long long)G.queues, K.name);
        if (print) continue;
        const BrickWant &W = kBrickWant[k];
        CHECK(key.want_dataflow == W.want_dataflow && key.chunk == W.chunk && key.gmax == W.gmax && P.glanes == W.glanes && P.nstages == W.nstages);
        CHECK((int)P.merge_stage.size() == W.points && P.nmb == W.nmb && P.tasks.size() == W.ntasks);
        CHECK(G.tasks == W.d.tasks && G.lists == W.d.lists && G.deps == W.d.deps && G.merge == W.d.merge && G.queues == W.d.queues);
    }
    // a direction that cannot be folded: the status, why, and no valid plan; no directions: an empty, valid plan
    {
        g_case = "failures";
        Dirs D = sets[0];
        D.theta[7] = 0.0;
        BrickPlan P;
        std::string why;
        const BrickKey key = key_of(def, 64, 8, 0, 8);
        CHECK(plan_bricks(BrickInputs{key, D.ndir(), D.phi.data(), D.theta.data(), D.w.data()}, P, &why) == FTTE_ERR_THETA && !P.valid && why.find("direction 7") == 0);
        CHECK(plan_bricks(BrickInputs{key, 0, nullptr, nullptr, nullptr}, P, &why) == FTTE_OK && P.valid && P.tasks.empty() && P.nstages == 0 && P.updates == 0);
        CHECK(P.glanes == 1 && P.stage_off == std::vector<size_t>(1, 0) && P.merge_stage.empty() && !P.persistent);
        Plan T;
        CHECK(plan_tiles(TileInputs{64, 1.0, 8, 1, 8, D.ndir(), D.phi.data(), D.theta.data(), D.w.data()}, T, &why) == FTTE_ERR_THETA && !T.valid && why.find("direction 7") == 0);
        CHECK(plan_tiles(TileInputs{64, 1.0, 8, 1, 8, 0, nullptr, nullptr, nullptr}, T, &why) == FTTE_OK && T.valid && T.items.empty() && T.launches.empty());
    }

    // ---- tiles: rows 4, 8, 16 and stacks 1, 2; with 48 directions 5 slots leave a short last batch (acc_base > 0)
    struct TileCase { const char *name; int n, rows, stack, slots; };
    const TileCase tiles[] = {
        {"tiles: n 64, rows 8, stack 1, slots 8", 64, 8, 1, 8},   {"tiles: n 5, rows 4, stack 1, slots 8", 5, 4, 1, 8},
        {"tiles: n 70, rows 16, stack 1, slots 8", 70, 16, 1, 8}, {"tiles: n 70, rows 8, stack 2, slots 5", 70, 8, 2, 5},
        {"tiles: n 130, rows 8, stack 1, slots 5", 130, 8, 1, 5}, {"tiles: n 130, rows 4, stack 2, slots 8", 130, 4, 2, 8},
        {"tiles: n 5, rows 16, stack 2, slots 5", 5, 16, 2, 5},
    };
    const size_t ntiles = sizeof tiles / sizeof tiles[0];
    CHECK(print || sizeof kTileWant / sizeof kTileWant[0] == ntiles);
    for (size_t k = 0; k < ntiles; ++k) {
        const TileCase &K = tiles[k];
        g_case = K.name;
        const Dirs &D = sets[1];
        const TileInputs in{K.n, 1.0, K.rows, K.stack, K.slots, D.ndir(), D.phi.data(), D.theta.data(), D.w.data()};
        Plan P;
        std::string why;
        CHECK(plan_tiles(in, P, &why) == 0);
        const TileWant G = check_tile_plan(P, in);
        CHECK((G.short_batches > 0) == (K.slots == 5));
        std::printf("    {%zu, %zu, %d, {0x%016llxull, 0x%016llxull, 0x%016llxull}}, // %s\n", G.nitems, G.nlaunches, G.short_batches, (unsigned long long)G.d.items,
                    (unsigned long long)G.d.launches, (unsigned long long)G.d.layers, K.name);
        if (print) continue;
        const TileWant &W = kTileWant[k];
        CHECK(G.nitems == W.nitems && G.nlaunches == W.nlaunches && G.short_batches == W.short_batches);
        CHECK(G.d.items == W.d.items && G.d.launches == W.d.launches && G.d.layers == W.d.layers);
    }
    std::printf("brick and tile plans under the sanitizers: ok\n");
    return 0;
}
