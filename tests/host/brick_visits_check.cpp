// Two passes of an izone per visit (radiativetransfer_amd/csrc/ftte_planner.cpp: link_visits, seat_stage_lists; ftte_bricks.h:
// BrickKey::duo, BrickOptions::visits) against a stub of the HIP runtime (tests/host/stub), under the address and
// undefined-behaviour sanitizers.  Direction sets: one direction per izone (24), HEALPix nside 2 (48), the benchmark's 96 (the
// first 96 NESTED pixels of nside 4) and all 192 of nside 4, on grids of 64 and 128 cells a side with 8 frequency groups.
// What a plan with visits must hold: every (pass, brick) once and in the list of its stage; every task in exactly one seat; a
// linked seat two passes of one izone on the same brick in the same stage, the owner first; a helper never stores or accumulates;
// exactly the first visitor of an accumulator's brick stores; upstream neighbours one stage earlier; merge points behind the last
// writers; 36 -> 23 visits for the 96 directions and 72 -> 46 for the 192; the LDS of a workgroup; and a key without the new
// member -- or a direction set without an izone of two passes -- plans what it planned before (the digests of brick_plan_check.cpp).
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
template <typename T> static uint64_t fnv_ints(uint64_t h, const std::vector<T> &v)
{
    for (const T &x : v) { const int64_t y = (int64_t)x; h = fnv(h, &y, 8); }
    return h;
}

struct Dirs { std::vector<double> phi, theta, w; int ndir() const { return (int)phi.size(); } };
static Dirs healpix(int nside, int64_t count) // the first `count` NESTED pixels, equal weights
{
    Dirs D;
    for (int64_t ipix = 0; ipix < count; ++ipix) {
        double p, t;
        CHECK(pix2ang_nest(nside, ipix, &p, &t) == 0);
        D.phi.push_back(p); D.theta.push_back(t); D.w.push_back(1.0 / (double)count);
    }
    return D;
}
static Dirs one_per_izone() // the first pixel of each izone at nside 4
{
    const Dirs all = healpix(4, 192);
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

// the digests of brick_plan_check.cpp that a plan of single passes enters with
struct Digests { uint64_t tasks, lists, merge; };
static Digests digests_of(const BrickPlan &P)
{
    Digests G;
    G.tasks = fnv(kSeed, P.tasks.data(), sizeof(BrickTask) * P.tasks.size());
    G.lists = fnv_ints(kSeed, P.stage_off);
    for (const auto &g : P.groups) G.lists = fnv_ints(G.lists, std::vector<int>{g.izone, g.layout, g.acc, g.offset, g.lane, (int)g.dirs.size()});
    G.lists = fnv_ints(G.lists, std::vector<int64_t>{P.nacc[0], P.nacc[1], P.nacc[2], P.vface_off, P.iface_off, P.uqface_off, P.face_elems, P.ut, P.uw, P.nslot, P.max_dirs,
                                                     P.glanes, P.nstages, P.updates});
    G.merge = fnv_ints(fnv_ints(fnv_ints(kSeed, P.merge_blocks), P.merge_stage), P.merge_off);
    return G;
}

static BrickPlan plan_of(const BrickKey &key, const Dirs &D)
{
    BrickPlan P;
    std::string why;
    const int rc = plan_bricks(BrickInputs{key, D.ndir(), D.phi.data(), D.theta.data(), D.w.data()}, P, &why);
    if (rc) std::fprintf(stderr, "ERROR %s: plan_bricks: %d %s\n", g_case, rc, why.c_str());
    CHECK(rc == 0 && P.valid);
    return P;
}

static size_t physical_brick(const BrickPlan &P, const BrickPlan::Group &G, int tu, int tv, int ti)
{
    const DirPlan &D0 = P.dirs[(size_t)G.dirs[0]];
    const int bu = D0.su < 0 ? P.ntu - 1 - tu : tu, bv = D0.sv < 0 ? P.ntv - 1 - tv : tv, bi = D0.si < 0 ? P.nti - 1 - ti : ti;
    return ((size_t)bi * P.ntv + bv) * P.ntu + bu;
}

// a plan with two passes per visit against the plan of single passes for the same inputs
static void check_visits(const BrickPlan &P, const BrickPlan &S, const BrickKey &key, int want_passes, int want_visits)
{
    const int n = key.n, ng = (int)P.groups.size(), ns = P.nstages;
    const size_t nb = (size_t)P.ntu * P.ntv * P.nti, nt = P.tasks.size();
    CHECK(P.duo && !S.duo && P.key.duo == 1 && ng == (int)S.groups.size() && ng == want_passes && P.nvisits == want_visits && S.nvisits == want_passes);
    CHECK(P.glanes == 1 && S.glanes == 1 && nt == (size_t)ng * nb && P.updates == S.updates && P.max_dirs == S.max_dirs);
    // ---- visits: the passes of an izone two by two, an odd last one alone; a visit where pass v of the single-pass plan stands
    int visits = 0, max_offset = 0;
    for (int g = 0; g < ng; ++g) {
        const BrickPlan::Group &G = P.groups[(size_t)g], &H = S.groups[(size_t)g];
        CHECK(G.izone == H.izone && G.layout == H.layout && G.acc == H.acc && G.dirs == H.dirs && G.lane == 0);
        int first = g;
        while (first > 0 && P.groups[(size_t)first - 1].izone == G.izone && P.groups[(size_t)first - 1].layout == G.layout) --first;
        const int p = g - first;
        const bool last = g + 1 == ng || P.groups[(size_t)g + 1].izone != G.izone || P.groups[(size_t)g + 1].layout != G.layout;
        CHECK(G.helper == (p % 2 == 1) && G.partner == (p % 2 ? g - 1 : last ? -1 : g + 1));
        CHECK(G.offset == S.groups[(size_t)first + (size_t)(p / 2)].offset); // (pass p / 2 exists: p / 2 <= p)
        if (G.partner >= 0) CHECK(P.groups[(size_t)G.partner].partner == g && P.groups[(size_t)G.partner].offset == G.offset && P.groups[(size_t)G.partner].acc == G.acc);
        if (!G.helper) ++visits;
        max_offset = std::max(max_offset, G.offset);
    }
    CHECK(visits == want_visits && ns == P.ntu + P.ntv + P.nti - 2 + max_offset && ns <= S.nstages);
    // ---- every (pass, brick) once, in the list of its stage; where it stands
    CHECK(P.stage_off.size() == (size_t)ns + 1 && P.stage_off[0] == 0 && P.stage_off.back() == nt);
    std::vector<int> stage_of((size_t)ng * nb, -1);
    std::vector<char> accumulates((size_t)ng * nb, 0);
    auto at = [&](int g, int tu, int tv, int ti) { return (size_t)g * nb + ((size_t)ti * P.ntv + tv) * P.ntu + tu; };
    for (int st = 0; st < ns; ++st) {
        CHECK(P.stage_off[(size_t)st] <= P.stage_off[(size_t)st + 1]);
        for (size_t q = P.stage_off[(size_t)st]; q < P.stage_off[(size_t)st + 1]; ++q) {
            const BrickTask &T = P.tasks[q];
            const int ti = T.ti & (kBrickAccumulate - 1);
            CHECK(T.group >= 0 && T.group < ng && T.tu >= 0 && T.tu < P.ntu && T.tv >= 0 && T.tv < P.ntv && ti < P.nti && !(T.ti & kBrickLinked));
            CHECK(st == T.tu + T.tv + ti + P.groups[(size_t)T.group].offset && stage_of[at(T.group, T.tu, T.tv, ti)] < 0);
            stage_of[at(T.group, T.tu, T.tv, ti)] = st;
            accumulates[at(T.group, T.tu, T.tv, ti)] = (T.ti & kBrickAccumulate) != 0;
        }
    }
    for (int s : stage_of) CHECK(s >= 0);
    // ---- upstream neighbours one stage earlier
    for (int g = 0; g < ng; ++g)
        for (int ti = 0; ti < P.nti; ++ti)
            for (int tv = 0; tv < P.ntv; ++tv)
                for (int tu = 0; tu < P.ntu; ++tu) {
                    const int st = stage_of[at(g, tu, tv, ti)];
                    if (tu > 0) CHECK(stage_of[at(g, tu - 1, tv, ti)] == st - 1);
                    if (tv > 0) CHECK(stage_of[at(g, tu, tv - 1, ti)] == st - 1);
                    if (ti > 0) CHECK(stage_of[at(g, tu, tv, ti - 1)] == st - 1);
                }
    // ---- a helper never stores or accumulates; of the others exactly the first visitor of an accumulator's brick stores, and
    // never two of them in one stage
    std::vector<std::vector<std::pair<int, size_t>>> visitors(3 * (size_t)kMaxAcc * nb);
    for (int g = 0; g < ng; ++g) {
        const BrickPlan::Group &G = P.groups[(size_t)g];
        for (int ti = 0; ti < P.nti; ++ti)
            for (int tv = 0; tv < P.ntv; ++tv)
                for (int tu = 0; tu < P.ntu; ++tu) {
                    if (G.helper) { CHECK(!accumulates[at(g, tu, tv, ti)]); continue; }
                    visitors[((size_t)G.layout * kMaxAcc + G.acc) * nb + physical_brick(P, G, tu, tv, ti)].push_back({stage_of[at(g, tu, tv, ti)], at(g, tu, tv, ti)});
                }
    }
    for (auto &V : visitors) {
        std::sort(V.begin(), V.end());
        for (size_t k = 0; k < V.size(); ++k) {
            if (k > 0) CHECK(V[k].first > V[k - 1].first);
            CHECK((accumulates[V[k].second] != 0) == (k > 0));
        }
    }
    // ---- seats: stage after stage; every task in exactly one place; linked seats; the seats with the most directions first
    CHECK(P.seat_off.size() == (size_t)ns + 1 && P.seat_off[0] == 0 && P.seat_off.back() == P.seats.size());
    std::vector<char> seated((size_t)ng * nb, 0);
    int linked = 0;
    for (int st = 0; st < ns; ++st) {
        CHECK(P.seat_off[(size_t)st] <= P.seat_off[(size_t)st + 1]);
        CHECK((P.seat_off[(size_t)st] == P.seat_off[(size_t)st + 1]) == (P.stage_off[(size_t)st] == P.stage_off[(size_t)st + 1]));
        size_t before = ~(size_t)0;
        int empties = 0;
        for (size_t q = P.seat_off[(size_t)st]; q < P.seat_off[(size_t)st + 1]; ++q) {
            const BrickSeat &Q = P.seats[q];
            const bool is_linked = (Q.place[0].ti & kBrickLinked) != 0;
            CHECK(is_linked == ((Q.place[1].ti & kBrickLinked) != 0));
            size_t ndirs = 0;
            for (int w = 0; w < 2; ++w) {
                const BrickTask &T = Q.place[w];
                if (T.group < 0) { CHECK(w == 1 && !is_linked && T.tu == 0 && T.tv == 0 && T.ti == 0); ++empties; continue; }
                const int ti = T.ti & (kBrickLinked - 1);
                CHECK(T.group < ng && T.tu >= 0 && T.tu < P.ntu && T.tv >= 0 && T.tv < P.ntv && ti >= 0 && ti < P.nti);
                const BrickPlan::Group &G = P.groups[(size_t)T.group];
                CHECK(stage_of[at(T.group, T.tu, T.tv, ti)] == st && !seated[at(T.group, T.tu, T.tv, ti)]++);
                CHECK(((T.ti & kBrickAccumulate) != 0) == (accumulates[at(T.group, T.tu, T.tv, ti)] != 0));
                CHECK(G.helper == (is_linked && w == 1) && (G.partner >= 0) == is_linked);
                ndirs += G.dirs.size();
            }
            if (is_linked) { // two passes of one izone on the same brick, the owner first; the helper's place carries no accumulate bit
                const BrickTask &A = Q.place[0], &B = Q.place[1];
                const BrickPlan::Group &GA = P.groups[(size_t)A.group], &GB = P.groups[(size_t)B.group];
                CHECK(GA.partner == B.group && GB.partner == A.group && GA.izone == GB.izone && GA.layout == GB.layout && GA.acc == GB.acc);
                CHECK(A.tu == B.tu && A.tv == B.tv && (A.ti & (kBrickLinked - 1)) == (B.ti & (kBrickLinked - 1)) && !(B.ti & kBrickAccumulate));
                ++linked;
            }
            CHECK(ndirs <= before);
            before = ndirs;
        }
        CHECK(empties <= 1);
    }
    for (char s : seated) CHECK(s == 1);
    CHECK(linked == P.nlinked && (size_t)linked == (size_t)(want_passes - want_visits) * nb);
    // ---- merge points behind the last writers (the helpers write nothing, and cross a brick in their owner's stage)
    {
        const int nmb = (n + kMergeBlock - 1) / kMergeBlock;
        const size_t nblk = (size_t)nmb * nmb * nmb;
        CHECK(P.nmb == nmb && P.merge_blocks.size() == nblk);
        std::vector<int> last(nblk, -1);
        for (size_t q = 0; q < nt; ++q) {
            const BrickTask &T = P.tasks[q];
            const BrickPlan::Group &G = P.groups[(size_t)T.group];
            if (G.helper) continue;
            const int ti = T.ti & (kBrickAccumulate - 1);
            const DirPlan &D0 = P.dirs[(size_t)G.dirs[0]];
            const int axis[3] = {G.layout, G.layout == 0 ? 1 : 0, G.layout == 2 ? 1 : 2};
            const int first[3] = {P.chunk * ti, kBrickRows * T.tv, 64 * T.tu}, size[3] = {P.chunk, kBrickRows, 64};
            const bool mirror[3] = {D0.si < 0, D0.sv < 0, D0.su < 0};
            int lo[3], hi[3];
            for (int a = 0; a < 3; ++a) {
                const int x0 = first[a], x1 = std::min(n, first[a] + size[a]) - 1;
                lo[axis[a]] = (mirror[a] ? n - 1 - x1 : x0) / kMergeBlock;
                hi[axis[a]] = (mirror[a] ? n - 1 - x0 : x1) / kMergeBlock;
            }
            for (int bi = lo[0]; bi <= hi[0]; ++bi)
                for (int bj = lo[1]; bj <= hi[1]; ++bj)
                    for (int bk = lo[2]; bk <= hi[2]; ++bk) { int &s = last[((size_t)bi * nmb + bj) * nmb + bk]; s = std::max(s, stage_of[at(T.group, T.tu, T.tv, ti)]); }
        }
        std::vector<int> times_block(nblk, 0);
        const size_t np = P.merge_stage.size();
        CHECK(np >= 1 && P.merge_off.size() == np + 1 && P.merge_off[0] == 0 && P.merge_off[np] == nblk && P.merge_stage[np - 1] == ns - 1);
        for (size_t m = 0; m < np; ++m) {
            CHECK(m == 0 || P.merge_stage[m] > P.merge_stage[m - 1]);
            for (size_t k = P.merge_off[m]; k < P.merge_off[m + 1]; ++k) {
                const int32_t b = P.merge_blocks[k];
                CHECK(b >= 0 && (size_t)b < nblk && times_block[(size_t)b]++ == 0 && last[(size_t)b] >= 0);
                CHECK(last[(size_t)b] <= P.merge_stage[m] && (m == 0 || last[(size_t)b] > P.merge_stage[m - 1]));
            }
        }
    }
    // ---- the LDS of a workgroup: the pad, two wavefronts' parked rays (4 KB per direction but one), 4 KB of exchange
    CHECK(brick_duo_lds(P.max_dirs, 0) == 2 * (size_t)(P.max_dirs - 1) * 4096 + 4096 && brick_duo_lds(P.max_dirs, 1024) == brick_duo_lds(P.max_dirs, 0) + 1024);
    CHECK(P.max_dirs == 3 && brick_duo_lds(3, 0) == 20480 && brick_duo_lds(kBrickMaxDirs, 0) <= 65536);
}

int main()
{
    const Dirs sets[4] = {one_per_izone(), healpix(2, 48), healpix(4, 96), healpix(4, 192)};
    const BrickOptions def = BrickOptions();
    const int nnu = 8;

    // ---- the step that sets the new member: only where the sweep has the form for it
    {
        g_case = "options";
        auto duo = [&](BrickOptions o, int n, int groups, int emit, bool plain) { BrickKey k = o.resolve(n, groups, emit); k.box = 1.0; o.visits(k, groups, emit, plain); return k.duo; };
        BrickOptions team0 = def, team2 = def, flow = def, chunk7 = def, share0 = def;
        team0.team = 0; team2.team = 2; flow.dataflow = 1; chunk7.chunk = 7; share0.share = 0;
        CHECK(def.resolve(64, 8, 0).duo == 0);                                          // resolve() alone never sets it
        CHECK(duo(def, 64, 8, 0, true) == 1 && duo(def, 128, 8, 0, true) == 1 && duo(def, 256, 8, 0, true) == 1);
        CHECK(duo(def, 64, 8, 0, false) == 0);                                          // tiled, atomic_acc, ablate or other waves
        CHECK(duo(def, 64, 4, 0, true) == 0 && duo(team0, 64, 2, 0, true) == 1);         // the pair form at up to four groups
        CHECK(duo(team2, 64, 8, 0, true) == 0 && duo(def, 64, 8, 1, true) == 0 && duo(def, 64, 8, 2, true) == 0);
        CHECK(duo(flow, 64, 8, 0, true) == 0 && duo(share0, 64, 8, 0, true) == 0);
        CHECK(duo(def, 70, 8, 0, true) == 0 && duo(def, 72, 8, 0, true) == 0 && duo(chunk7, 64, 8, 0, true) == 0);
        BrickKey a = def.resolve(64, 8, 0), b = a;
        b.duo = 1;
        CHECK(!(a == b));
    }

    // what brick_plan_check.cpp pins for default options, 8 frequency groups, n = 64: 24, 48 and 192 directions
    const Digests pinned[3] = {{0x72d8f99d96e813a5ull, 0x30cc9f4103a08779ull, 0x38a69c4ffe6bc5c7ull},
                               {0x8fd646dc32afd825ull, 0x941e7473e1b7cd1bull, 0x38a69c4ffe6bc5c7ull},
                               {0xcc7d86b15b565165ull, 0x1384a518ca2639efull, 0xaa64844430e6d017ull}};
    struct Case { const char *name; int set, n, passes, visits, pin; };
    const Case cases[] = {
        {"24 directions, n 64", 0, 64, 24, 24, 0},   {"24 directions, n 128", 0, 128, 24, 24, -1},
        {"48 directions, n 64", 1, 64, 24, 24, 1},   {"48 directions, n 128", 1, 128, 24, 24, -1},
        {"96 directions, n 64", 2, 64, 36, 23, -1},  {"96 directions, n 128", 2, 128, 36, 23, -1},
        {"192 directions, n 64", 3, 64, 72, 46, 2},  {"192 directions, n 128", 3, 128, 72, 46, -1},
    };
    for (const Case &K : cases) {
        g_case = K.name;
        const Dirs &D = sets[K.set];
        BrickKey single = def.resolve(K.n, nnu, 0), key;
        single.box = 1.0;
        key = single;
        def.visits(key, nnu, 0, true);
        CHECK(single.duo == 0 && key.duo == 1);
        // a key without the new member: the plan of before
        const BrickPlan S = plan_of(single, D);
        const Digests GS = digests_of(S);
        CHECK(!S.duo && S.seats.empty() && S.seat_off.empty() && S.nlinked == 0 && (int)S.groups.size() == K.passes);
        for (const auto &G : S.groups) CHECK(G.partner < 0 && !G.helper);
        if (K.pin >= 0) CHECK(GS.tasks == pinned[K.pin].tasks && GS.lists == pinned[K.pin].lists && GS.merge == pinned[K.pin].merge);
        const BrickPlan P = plan_of(key, D);
        if (K.visits == K.passes) { // no izone with two passes: the same plan, no seats
            const Digests GP = digests_of(P);
            CHECK(!P.duo && P.seats.empty() && P.nlinked == 0 && P.nvisits == K.passes && GP.tasks == GS.tasks && GP.lists == GS.lists && GP.merge == GS.merge);
            continue;
        }
        check_visits(P, S, key, K.passes, K.visits);
        std::printf("%s: %d passes in %d visits, %d stages (single passes: %d), %zu seats, %d of them linked\n", K.name, K.passes, P.nvisits, P.nstages, S.nstages,
                    P.seats.size(), P.nlinked);
    }
    std::printf("brick visits under the sanitizers: ok\n");
    return 0;
}
