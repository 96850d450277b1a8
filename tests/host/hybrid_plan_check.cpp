// The hybrid sweep's planner (radiativetransfer_amd/csrc/ftte_planner.cpp: plan_hybrid) and the owners of the refined-grid sweeps
// (ftte_forests.h, ftte_hybrid.h) against a stub of the HIP runtime (tests/host/stub), under the address and undefined-behaviour
// sanitizers with leak detection.  Four trees, one direction per izone (the first pixel of each at HEALPix level 3), chunk 4:
// what the bricks cover, in which order the lists hold them, who stores and who accumulates, the fine block's lists, the owners'
// releases and the graph signature; and FNV-1a-64 digests of the plan pinned to what the planner produced before it was split.
#include <array>
#include <cstdio>
#include <cstdlib>
#include <map>
#include <set>

#include "ftte_geometry.h"
#include "ftte_hybrid.h"

using namespace ftte;

#define CHECK(cond)                                                                                                \
    do {                                                                                                           \
        if (!(cond)) { std::fprintf(stderr, "ERROR %s:%d (%s): %s\n", __FILE__, __LINE__, g_case, #cond); std::exit(1); } \
    } while (0)
static const char *g_case = "";

using Cell = std::array<int, 3>;

// the depth-first leaf list of an n^3 base grid whose cells `blocks` (0-based) are refined `depth` times
static std::vector<int32_t> levels_of(int n, const std::set<Cell> &blocks, int depth)
{
    std::vector<int32_t> out;
    size_t leaves = 1;
    for (int k = 0; k < depth; ++k) leaves *= 8;
    for (int i = 0; i < n; ++i)
        for (int j = 0; j < n; ++j)
            for (int k = 0; k < n; ++k) {
                if (blocks.count({i, j, k})) out.insert(out.end(), leaves, depth);
                else out.push_back(0);
            }
    return out;
}
static std::set<Cell> cube(Cell lo, int qa, int qb, int qc)
{
    std::set<Cell> s;
    for (int a = 0; a < qa; ++a) for (int b = 0; b < qb; ++b) for (int c = 0; c < qc; ++c) s.insert({lo[0] + a, lo[1] + b, lo[2] + c});
    return s;
}

static uint64_t fnv(uint64_t h, const void *p, size_t bytes)
{
    const unsigned char *b = (const unsigned char *)p;
    for (size_t i = 0; i < bytes; ++i) { h ^= b[i]; h *= 1099511628211ull; }
    return h;
}
constexpr uint64_t kSeed = 14695981039346656037ull;
struct Digests { uint64_t tasks, stage_off, pass_at, cells, rec, active, exports, imports, fine_tasks, fine_stage_off; };
static Digests digests_of(const HybridPlan &H)
{
    Digests D;
    D.tasks = fnv(kSeed, H.bricks.tasks.data(), sizeof(BrickTask) * H.bricks.tasks.size());
    std::vector<uint64_t> so(H.stage_off.begin(), H.stage_off.end());
    D.stage_off = fnv(kSeed, so.data(), 8 * so.size());
    D.pass_at = kSeed;
    for (const auto &at : H.pass_at) { std::vector<int32_t> v(at.begin(), at.end()); D.pass_at = fnv(D.pass_at, v.data(), 4 * v.size()); }
    D.cells = fnv(kSeed, H.cells.data(), 4 * H.cells.size());
    D.rec = D.active = D.exports = D.imports = kSeed;
    for (const HybridPlan::Dir &d : H.dirs) {
        D.rec = fnv(D.rec, d.rec.data(), sizeof(SegRec) * d.rec.size());
        D.active = fnv(D.active, d.active.data(), d.active.size());
        D.exports = fnv(D.exports, d.exports.data(), sizeof(AmrExport) * d.exports.size());
        D.imports = fnv(D.imports, d.imports.data(), sizeof(AmrImport) * d.imports.size());
    }
    D.fine_tasks = fnv(kSeed, H.fine.plan.tasks.data(), sizeof(BrickTask) * H.fine.plan.tasks.size());
    std::vector<uint64_t> fso(H.fine.stage_off.begin(), H.fine.stage_off.end());
    D.fine_stage_off = fnv(kSeed, fso.data(), 8 * fso.size());
    return D;
}

struct Dirs { std::vector<double> phi, theta, w; };
static Dirs one_per_izone()
{
    Dirs D;
    D.phi.assign(24, 0); D.theta.assign(24, 0); D.w.assign(24, 1.0 / 24);
    bool have[25] = {};
    for (int64_t ipix = 0; ipix < 192; ++ipix) { // level 3: nside 4
        double p, t, fp, ft;
        int izone = 0;
        CHECK(pix2ang_nest(4, ipix, &p, &t) == 0 && fold_direction(p, t, &fp, &ft, &izone) == 0 && izone >= 1 && izone <= 24);
        if (!have[izone]) { have[izone] = true; D.phi[(size_t)izone - 1] = p; D.theta[(size_t)izone - 1] = t; }
    }
    for (int z = 1; z <= 24; ++z) CHECK(have[z]);
    return D;
}

// a task of the plan, decoded: its group, brick, lanes, list and pipeline
struct PieceAt { int g, tu, tv, ti, lo, hi, box, pipe; size_t list; bool masked, accumulates; };

// sweep-frame cell (i, j, k), 1-based, of group `izone` -> base cell in storage order
static int64_t base_cell(int n, const ZoneMap &zm, int i, int j, int k)
{
    const int sw[3] = {i, j, k};
    int st[3];
    for (int a = 0; a < 3; ++a) st[a] = zm.mirror[a] ? n + 1 - sw[zm.src[a]] : sw[zm.src[a]];
    return ((int64_t)(st[0] - 1) * n + (st[1] - 1)) * n + (st[2] - 1);
}
static void leaves_under(const AmrTree &T, int32_t node, std::vector<int32_t> *out)
{
    if (T.child0[(size_t)node] < 0) { out->push_back(T.leaf[(size_t)node]); return; }
    for (int k = 0; k < 8; ++k) leaves_under(T, T.child0[(size_t)node] + k, out);
}

static void check_plan(const AmrTree &tree, const HybridInputs &in, const HybridPlan &H)
{
    const BrickPlan &P = H.bricks;
    const int n = in.n, ng = (int)P.groups.size();
    const size_t nlists = (size_t)H.nhalves * H.nlist;
    CHECK(H.valid && H.worthwhile && (int)H.regions.size() == ng && (int)H.dirs.size() == in.ndir);
    // ---- lists: monotone offsets that cover the tasks; lane ranges only in the masked half
    CHECK(H.stage_off.size() == 2 * nlists + 1 && H.stage_off[0] == 0 && H.stage_off.back() == P.tasks.size());
    std::vector<PieceAt> pieces;
    for (size_t L = 0; L < 2 * nlists; ++L) {
        CHECK(H.stage_off[L] <= H.stage_off[L + 1]);
        for (size_t q = H.stage_off[L]; q < H.stage_off[L + 1]; ++q) {
            const BrickTask &T = P.tasks[q];
            PieceAt A;
            A.masked = L >= nlists;
            A.pipe = (int)((L % nlists) / H.nlist); A.list = (L % nlists) % H.nlist;
            A.g = T.group & kBrickGroupMask; A.tu = (uint16_t)T.tu & kBrickTuMask; A.tv = T.tv & kBrickTvMask; A.ti = T.ti & (kBrickAccumulate - 1);
            A.lo = (uint16_t)T.tu >> kBrickLaneLoShift; A.hi = (T.group >> kBrickLaneHiShift) & 63; A.box = T.tv >> kBrickBoxShift;
            A.accumulates = (T.ti & kBrickAccumulate) != 0;
            if (!A.masked) { CHECK(A.lo == 0 && A.hi == 0 && A.box == 0); A.hi = 63; }
            CHECK(A.g < ng && A.tu < P.ntu && A.tv < P.ntv && A.ti < P.nti && A.lo <= A.hi);
            pieces.push_back(A);
        }
    }
    // ---- accumulators: the groups of one are in one pipeline; half_dirs partitions the directions
    std::vector<int> pipe_of(ng, -1);
    for (const PieceAt &A : pieces) { CHECK(pipe_of[A.g] < 0 || pipe_of[A.g] == A.pipe); pipe_of[A.g] = A.pipe; }
    std::map<int, int> pipe_of_acc;
    for (int g = 0; g < ng; ++g) {
        const int a = P.groups[g].layout * kMaxAcc + P.groups[g].acc;
        if (pipe_of[g] < 0) continue;
        CHECK(!pipe_of_acc.count(a) || pipe_of_acc[a] == pipe_of[g]);
        pipe_of_acc[a] = pipe_of[g];
    }
    std::vector<int> seen_dir(in.ndir, 0);
    CHECK((int)H.half_dirs.size() == H.nhalves);
    for (int h = 0; h < H.nhalves; ++h)
        for (int d : H.half_dirs[(size_t)h]) { CHECK(d >= 0 && d < in.ndir && !seen_dir[d]++); }
    for (int d = 0; d < in.ndir; ++d) CHECK(seen_dir[d] == 1);
    for (int g = 0; g < ng; ++g)
        for (int d : P.groups[g].dirs) {
            bool found = false;
            for (int x : H.half_dirs[(size_t)pipe_of[g]]) found = found || x == d;
            CHECK(found);
        }
    // exactly the tasks of the earliest list of an accumulator and brick store; no list holds a brick for two of its groups
    {
        std::map<std::array<int64_t, 2>, size_t> first;                  // (accumulator, physical brick) -> earliest list
        std::map<std::array<int64_t, 3>, int> holder;                    // (accumulator, physical brick, list) -> group
        auto key_of = [&](const PieceAt &A) {
            const BrickPlan::Group &G = P.groups[A.g];
            const DirPlan &D0 = P.dirs[G.dirs[0]];
            const int bu = D0.su < 0 ? P.ntu - 1 - A.tu : A.tu, bv = D0.sv < 0 ? P.ntv - 1 - A.tv : A.tv, bi = D0.si < 0 ? P.nti - 1 - A.ti : A.ti;
            return std::array<int64_t, 2>{G.layout * kMaxAcc + G.acc, ((int64_t)bi * P.ntv + bv) * P.ntu + bu};
        };
        for (const PieceAt &A : pieces) {
            const auto k = key_of(A);
            if (!first.count(k) || A.list < first[k]) first[k] = A.list;
            const std::array<int64_t, 3> hk = {k[0], k[1], (int64_t)A.list};
            CHECK(!holder.count(hk) || holder[hk] == A.g);
            holder[hk] = A.g;
        }
        for (const PieceAt &A : pieces) CHECK(A.accumulates == (A.list > first[key_of(A)]));
    }
    // ---- coverage and order, group by group
    int64_t updates = 0;
    std::vector<uint8_t> in_any((size_t)tree.ncell, 0);
    std::vector<std::vector<uint8_t>> in_own((size_t)ng);
    for (int g = 0; g < ng; ++g) {
        const std::vector<ForestRegion> &RG = H.regions[(size_t)g];
        ZoneMap zm;
        zone_map(P.groups[g].izone, &zm);
        const bool u_is_k = RG.empty() ? true : RG[0].u_is_k;
        auto ijk = [&](int u, int v, int i) { return u_is_k ? Cell{i, v, u} : Cell{i, u, v}; };
        auto region_at = [&](int u, int v, int i) -> const ForestRegion * {
            const Cell c = ijk(u, v, i);
            for (const ForestRegion &R : RG) if (R.contains(c[0], c[1], c[2])) return &R;
            return nullptr;
        };
        // every unrefined base cell outside the boxes in exactly one task's lanes, the cells inside in none
        std::vector<uint8_t> count((size_t)n * n * n, 0);
        for (const PieceAt &A : pieces) {
            if (A.g != g) continue;
            for (int i = P.chunk * A.ti + 1; i <= std::min(n, P.chunk * (A.ti + 1)); ++i)
                for (int v = kBrickRows * A.tv + 1; v <= std::min(n, kBrickRows * (A.tv + 1)); ++v)
                    for (int u = 64 * A.tu + A.lo + 1; u <= std::min(n, 64 * A.tu + A.hi + 1); ++u) {
                        ++count[((size_t)(i - 1) * n + (v - 1)) * n + (u - 1)];
                        updates += (int64_t)P.groups[g].dirs.size();
                    }
        }
        in_own[(size_t)g].assign((size_t)tree.ncell, 0);
        for (int i = 1; i <= n; ++i)
            for (int v = 1; v <= n; ++v)
                for (int u = 1; u <= n; ++u) {
                    const ForestRegion *R = region_at(u, v, i);
                    const Cell c = ijk(u, v, i);
                    const int64_t b = base_cell(n, zm, c[0], c[1], c[2]);
                    CHECK(count[((size_t)(i - 1) * n + (v - 1)) * n + (u - 1)] == (R ? 0 : 1));
                    if (!R) { CHECK(tree.child0[(size_t)b] < 0); continue; } // (what the bricks sweep is unrefined)
                    if (R->in_fine(c[0], c[1], c[2])) continue;               // (the fine block's leaves: its own bricks')
                    std::vector<int32_t> leaves;
                    leaves_under(tree, (int32_t)b, &leaves);
                    for (int32_t q : leaves) in_own[(size_t)g][(size_t)q] = in_any[(size_t)q] = 1;
                }
        // order: upstream pieces that share lanes in strictly earlier lists; feeders of a box before its pass, what lies behind it after
        std::map<std::array<int, 3>, std::vector<const PieceAt *>> at;
        for (const PieceAt &A : pieces) if (A.g == g) at[{A.tu, A.tv, A.ti}].push_back(&A);
        const std::vector<int> &pass_at = H.pass_at[(size_t)pipe_of[g]];
        for (const PieceAt &A : pieces) {
            if (A.g != g) continue;
            const int u0 = 64 * A.tu + A.lo + 1, u1 = std::min(n, 64 * A.tu + A.hi + 1), v0 = kBrickRows * A.tv + 1, v1 = std::min(n, kBrickRows * (A.tv + 1)),
                      i0 = P.chunk * A.ti + 1, i1 = std::min(n, P.chunk * (A.ti + 1));
            if (A.lo == 0 && A.tu > 0) for (const PieceAt *B : at[{A.tu - 1, A.tv, A.ti}]) if (B->hi == 63) CHECK(B->list < A.list);
            if (A.tv > 0) for (const PieceAt *B : at[{A.tu, A.tv - 1, A.ti}]) if (B->lo <= A.hi && B->hi >= A.lo) CHECK(B->list < A.list);
            if (A.ti > 0) for (const PieceAt *B : at[{A.tu, A.tv, A.ti - 1}]) if (B->lo <= A.hi && B->hi >= A.lo) CHECK(B->list < A.list);
            for (int u = u0; u <= u1; ++u) { // (the boxes end on brick boundaries along v and the march axis: one row and layer stand for all)
                if (v1 < n) if (const ForestRegion *R = region_at(u, v1 + 1, i0)) CHECK((int)A.list < pass_at[(size_t)R->pass]);
                if (i1 < n) if (const ForestRegion *R = region_at(u, v0, i1 + 1)) CHECK((int)A.list < pass_at[(size_t)R->pass]);
                if (v0 > 1) if (const ForestRegion *R = region_at(u, v0 - 1, i0)) CHECK((int)A.list >= pass_at[(size_t)R->pass]);
                if (i0 > 1) if (const ForestRegion *R = region_at(u, v0, i0 - 1)) CHECK((int)A.list >= pass_at[(size_t)R->pass]);
            }
            if (u1 < n) if (const ForestRegion *R = region_at(u1 + 1, v0, i0)) CHECK((int)A.list < pass_at[(size_t)R->pass]);
            if (u0 > 1) if (const ForestRegion *R = region_at(u0 - 1, v0, i0)) CHECK((int)A.list >= pass_at[(size_t)R->pass]);
        }
    }
    CHECK(updates == H.brick_updates);
    if (!H.slots)
        for (const auto &at : H.pass_at) for (int k = 0; k < H.npass; ++k) CHECK(at[(size_t)k] == (k + 1) * (int)H.phase1_stages);
    // ---- cells: each leaf inside a box of any direction exactly once; bit 2 of a direction's byte clear exactly inside its own boxes
    size_t want = 0;
    for (uint8_t x : in_any) want += x;
    CHECK(H.cells.size() == want);
    for (size_t p = 0; p < H.cells.size(); ++p) CHECK(in_any[(size_t)H.cells[p]] && (p == 0 || H.cells[p - 1] < H.cells[p]));
    for (int g = 0; g < ng; ++g)
        for (int d : P.groups[g].dirs) {
            const HybridPlan::Dir &D = H.dirs[(size_t)d];
            CHECK(D.active.size() == H.cells.size());
            for (size_t p = 0; p < H.cells.size(); ++p) CHECK(((D.active[p] & 4) == 0) == (in_own[(size_t)g][(size_t)H.cells[p]] != 0));
        }
    // ---- the fine block: the base plan's groups, every (group, fine brick) once in list pipeline * nstages + tu + tv + ti, a
    // bijection from fine cells onto the block's leaves
    if (H.fine.active) {
        const HybridPlan::Fine &F = H.fine;
        const BrickPlan &Q = F.plan;
        CHECK(Q.groups.size() == P.groups.size() && F.stage_off.size() == (size_t)H.nhalves * F.nstages + 1 && F.stage_off.back() == Q.tasks.size());
        std::set<std::array<int, 4>> seen;
        for (size_t l = 0; l + 1 < F.stage_off.size(); ++l)
            for (size_t q = F.stage_off[l]; q < F.stage_off[l + 1]; ++q) {
                const BrickTask &T = Q.tasks[q];
                CHECK(seen.insert({T.group, T.tu, T.tv, T.ti}).second);
                CHECK(l == (size_t)pipe_of[T.group] * F.nstages + (size_t)(T.tu + T.tv + T.ti));
            }
        CHECK(seen.size() == Q.groups.size() * (size_t)Q.ntu * Q.ntv * Q.nti);
        std::vector<int32_t> block;
        for (int a = 0; a < F.n / 2; ++a) for (int b = 0; b < F.n / 2; ++b) for (int c = 0; c < F.n / 2; ++c)
            leaves_under(tree, (int32_t)(((int64_t)(F.lo[0] - 1 + a) * n + (F.lo[1] - 1 + b)) * n + (F.lo[2] - 1 + c)), &block);
        std::vector<int32_t> mapped(F.leaf_of_fine);
        std::sort(block.begin(), block.end()); std::sort(mapped.begin(), mapped.end());
        CHECK(mapped.size() == (size_t)F.n * F.n * F.n && mapped == block && std::adjacent_find(mapped.begin(), mapped.end()) == mapped.end());
    }
}

// the owners: a plan on the device and off it again, and the signature of what a captured sweep names
static void check_device(HybridPlan H, const Dirs &D)
{
    const long base = stub().live;
    {
        HybridDevice V;
        ForestScratch S;
        BrickTables T;
        CHECK(V.upload(H, D.w, 7) == hipSuccess && V.cells_id == 7 && V.ncells == (int64_t)H.cells.size() && V.dirs.size() == D.w.size());
        CHECK(H.dirs[0].rec.empty() && !V.dirs[0].depth_off.empty() && V.dirs[0].w == D.w[0]); // (the host copies are gone)
        CHECK(to_device(V.leaf_of_base, std::vector<int32_t>(100, 1)) == hipSuccess && T.upload(H.bricks) == hipSuccess);
        CHECK(V.base_kappa.reserve(64) == hipSuccess);
        hipError_t e;
        CHECK(S.reserve_batch(30, 24, 1024, 0.6, false, &e) == 24 && S.dirs.reserve(24) == hipSuccess && S.tables.reserve(48) == hipSuccess);
        CHECK(stub().live > base);
        auto signature = [&] {
            std::vector<uintptr_t> sig;
            V.sign(sig, H.fine.active, H.fine.plan.nacc); S.sign(sig); sign_tables(T, sig);
            return sig;
        };
        const std::vector<uintptr_t> sig = signature();
        auto covers = [&](const void *p) { return std::find(sig.begin(), sig.end(), (uintptr_t)p) != sig.end(); };
        CHECK(covers(V.cells.get()) && covers(V.leaf_of_base.get()) && covers(V.dirs[3].rec.get()) && covers(V.dirs[3].active.get()) && covers(V.dirs[3].exports.get()));
        CHECK(covers(S.Iout.get()) && covers(S.mean.get()) && covers(S.dirs.get()) && covers(S.tables.get()) && covers(T.tasks.get()) && covers(T.groups.get()));
        for (int l = 0; l < 3; ++l) CHECK(covers(V.base_kappa[l]));
        if (H.fine.active) CHECK(covers(V.leaf_of_fine.get()) && covers(V.fine_tables.tasks.get()));
        // a buffer it covers reallocated: another signature (an address that stayed the same would name the same memory)
        const double *was = S.Iout;
        CHECK(S.reserve_batch(60, 24, 1024, 0.6, false, &e) == 24 && (S.Iout.get() == was || signature() != sig));
        const double *layout = V.base_kappa[1];
        CHECK(V.base_kappa.reserve(128) == hipSuccess && (V.base_kappa[1] == layout || signature() != sig));
        const long before_drop = stub().live;
        V.drop_grid();
        CHECK(!V.cells && !V.leaf_of_base && V.dirs.empty() && V.ncells == 0 && stub().live < before_drop);
        CHECK(stub().live == base + 3 /* base_kappa */ + 4 /* scratch */ + 2 /* tables */);
    }
    CHECK(stub().live == base);
}

static void check_scratch()
{
    g_case = "scratch";
    const long base = stub().live;
    {
        ForestScratch S;
        hipError_t e = hipSuccess;
        // a failed allocation, of the first array or of the second: both empty, capacity 0, nothing alive
        for (int k = 1; k <= 2; ++k) {
            stub().fail_countdown = k;
            CHECK(S.reserve_batch(100, 24, 1024, 0.6, false, &e) == 0 && e != hipSuccess);
            CHECK(!S.Iout && !S.mean && S.Iout.capacity() == 0 && S.mean.capacity() == 0 && S.capacity() == 0 && stub().live == base);
        }
        // the whole-tree path halves the batch and tries again; with one direction left it gives up
        stub().fail_countdown = 1;
        CHECK(S.reserve_batch(100, 24, 96, 0.9, true, &e) == 12 && S.capacity() == 1200 && stub().live == base + 2);
        S.drop();
        stub().fail_countdown = 1;
        CHECK(S.reserve_batch(100, 1, 96, 0.9, true, &e) == 0 && S.capacity() == 0 && stub().live == base);
        // the free memory bounds the batch: 0.6 of 16000 bytes hold 6 directions of two arrays of 100 doubles, 0.9 hold 9
        stub().free_bytes = 16000;
        CHECK(S.reserve_batch(100, 24, 1024, 0.6, false, &e) == 6 && S.capacity() == 600);
        S.drop();
        CHECK(S.reserve_batch(100, 24, 96, 0.9, true, &e) == 9 && S.capacity() == 900);
        // enough capacity: the buffers stay, and the batch is what they hold of the new size (at most `most`)
        const double *was = S.Iout;
        CHECK(S.fits(50, 12, 1024) && S.reserve_batch(50, 12, 1024, 0.6, false, &e) == 18 && S.Iout.get() == was);
        CHECK(S.reserve_batch(50, 12, 16, 0.6, false, &e) == 16 && S.Iout.get() == was);
        CHECK(!S.fits(100, 24, 1024));
        stub().free_bytes = (size_t)1 << 30;
    }
    CHECK(stub().live == base);
    ForestCache C;
    C.dirs.resize(3); C.key = {1.0, 2.0};
    CHECK(C.current({1.0, 2.0}, 3) && !C.current({1.0, 2.0}, 2) && !C.current({1.0, 2.5}, 3));
    C.drop();
    CHECK(C.dirs.empty() && !C.current({1.0, 2.0}, 3));
}

struct Case { const char *name; int n; std::set<Cell> blocks; int depth; int slots, pipelines, fine_block, min_boxes, min_passes; Digests want; };

static void merge(std::set<Cell> &a, const std::set<Cell> &b) { a.insert(b.begin(), b.end()); }

int main()
{
    const Dirs D = one_per_izone();
    // three 2^3 patches along the body diagonal, far enough apart for the boxes of an izone not to be merged
    std::set<Cell> diagonal = cube({6, 6, 6}, 2, 2, 2);
    merge(diagonal, cube({30, 30, 30}, 2, 2, 2));
    merge(diagonal, cube({54, 54, 54}, 2, 2, 2));
    // The digests are those of the planner before it was split into steps (build_hybrid_plan of the parent commit), taken
    // there from the same four trees and directions.
    const Case cases[] = {
        {"case 1: 3 x 2 x 4 patch, one level, n = 64", 64, cube({30, 31, 33}, 3, 2, 4), 1, 1, 3, 0, 1, 1,
         {0xc134c1075f5a0aa1ull, 0x5370c8e372c39a13ull, 0x567e7feac5658322ull, 0x3472c03162278be5ull, 0x3b66158d004333a1ull, 0xf33d01bd5f4aa429ull,
          0x27e3aa5bf02db852ull, 0xcbf29ce484222325ull, 0xcbf29ce484222325ull, 0xcbf29ce484222325ull}},
        {"case 2: ragged patch, two levels, n = 72", 72, {{40, 41, 20}, {41, 41, 20}, {40, 42, 21}}, 2, 1, 3, 0, 1, 1,
         {0x76f9fbeb451417f9ull, 0x349d8f034e281fb8ull, 0xe1a767668e5d88aeull, 0x81bddb14bea1c189ull, 0x02de9a80d90a4ed6ull, 0x56b5625f2a10f580ull,
          0xc2b7354f0072ec74ull, 0xcbf29ce484222325ull, 0xcbf29ce484222325ull, 0xcbf29ce484222325ull}},
        {"case 3: fully refined 32^3 cube, n = 64", 64, cube({8, 24, 12}, 32, 32, 32), 1, 1, 3, 64, 1, 1,
         {0xc71c7880b0d2ba39ull, 0xc404bb693a9b834eull, 0x567e7feac5658322ull, 0xe2c2718085cbd2a9ull, 0x08ed3a62825a42ccull, 0xcb5ed9515fc1c765ull,
          0xb82b2d45ec1f6b68ull, 0x55d2f938272ab39dull, 0x588c72ea378a0e65ull, 0xf96bc6729dc9d974ull}},
        {"case 4: three patches on the diagonal, slots", 64, diagonal, 1, 1, 3, 0, 2, 2,
         {0x7a000f27a5e33a99ull, 0xc1866690462ec362ull, 0xb2a55c56c9586b06ull, 0x1490577ec80d71ffull, 0x901213dbf311374aull, 0xc741c45644bfd8ddull,
          0xdd3e6000fccc22deull, 0xcbf29ce484222325ull, 0xcbf29ce484222325ull, 0xcbf29ce484222325ull}},
        {"case 4: three patches on the diagonal, phases", 64, diagonal, 1, 0, 3, 0, 2, 2,
         {0x26086e5d70f4ba99ull, 0x19d910f46e69a371ull, 0x8b85f0805c5348c9ull, 0x1490577ec80d71ffull, 0x901213dbf311374aull, 0xc741c45644bfd8ddull,
          0xdd3e6000fccc22deull, 0xcbf29ce484222325ull, 0xcbf29ce484222325ull, 0xcbf29ce484222325ull}},
    };
    for (const Case &K : cases) {
        g_case = K.name;
        const std::vector<int32_t> level = levels_of(K.n, K.blocks, K.depth);
        AmrTree tree;
        CHECK(tree.build(K.n, (int64_t)level.size(), level.data()).empty());
        HybridOptions opt;
        opt.slots = K.slots; opt.pipelines = K.pipelines;
        const HybridInputs in{K.n, 1.0, &tree, opt, 4, 3, 2, 24, D.phi.data(), D.theta.data(), D.w.data()};
        HybridPlan H;
        std::string why;
        const int rc = plan_hybrid(in, H, &why);
        if (rc) std::fprintf(stderr, "ERROR %s: plan_hybrid: %d %s\n", K.name, rc, why.c_str());
        CHECK(rc == 0);
        CHECK(H.slots == (K.slots && H.npass > 1) && H.nhalves == K.pipelines && (H.fine.active ? H.fine.n : 0) == K.fine_block);
        CHECK(H.brick_plans_made == (K.fine_block ? 2 : 1) && H.forests_linked);
        // boxes and passes, izone by izone (a direction's forest has a pass per level of its boxes)
        int two_boxes = 0, two_passes = 0;
        for (size_t g = 0; g < H.bricks.groups.size(); ++g) {
            if ((int)H.regions[g].size() >= K.min_boxes) ++two_boxes;
            int levels = 0;
            for (const ForestRegion &R : H.regions[g]) levels = std::max(levels, R.pass + 1);
            if (levels >= K.min_passes) ++two_passes;
        }
        std::printf("%s: %d boxes at most, %d passes, %zu tasks, %zu lists, %zu leaves in boxes; %d / %d of 24 izones with %d boxes / passes or more\n", K.name, H.most_boxes,
                    H.npass, H.bricks.tasks.size(), H.stage_off.size() - 1, H.cells.size(), two_boxes, two_passes, K.min_boxes);
        // (Case 4: every izone has its boxes.  The patches lie at least three 8-cell blocks apart on every axis -- nearer ones are one
        // cluster -- so their boxes are strictly ordered along v and along the march axis, and a 64^3 grid has one brick along u: a box
        // lies behind another exactly in the twelve izones in which the diagonal runs the same way along v and the march axis.)
        CHECK(two_boxes == 24 && two_passes >= 12 && H.npass >= K.min_passes && H.most_boxes >= K.min_boxes);
        check_plan(tree, in, H);
        const Digests G = digests_of(H);
        std::printf("  tasks %016llx stage_off %016llx pass_at %016llx cells %016llx rec %016llx active %016llx exports %016llx imports %016llx fine %016llx %016llx\n",
                    (unsigned long long)G.tasks, (unsigned long long)G.stage_off, (unsigned long long)G.pass_at, (unsigned long long)G.cells, (unsigned long long)G.rec,
                    (unsigned long long)G.active, (unsigned long long)G.exports, (unsigned long long)G.imports, (unsigned long long)G.fine_tasks, (unsigned long long)G.fine_stage_off);
        CHECK(G.tasks == K.want.tasks && G.stage_off == K.want.stage_off && G.pass_at == K.want.pass_at && G.cells == K.want.cells);
        CHECK(G.rec == K.want.rec && G.active == K.want.active && G.exports == K.want.exports && G.imports == K.want.imports);
        CHECK(G.fine_tasks == K.want.fine_tasks && G.fine_stage_off == K.want.fine_stage_off);
        check_device(std::move(H), D);
    }
    check_scratch();
    std::printf("hybrid plan under the sanitizers: ok\n");
    return 0;
}
