// ftte_planner.cpp -- the planners that read no context: one direction's layer tables (plan_direction), the groups, accumulators
// and face blocks of a brick plan (plan_brick_groups), the one builder of stage-ordered task lists (build_task_lists: count, offsets,
// fill, and who stores and who accumulates), the uniform grid's brick plan in steps (plan_bricks: groups, lanes of groups, stage
// lists, dependencies, merge points, queues) and its tile plan (plan_tiles), and the hybrid sweep's plan for a refined cell array
// (plan_hybrid: boxes around the clusters of refined cells, pipelines, the fine block, slots, task lists, the forests restricted to
// the boxes).  Pure host work against the owners' headers only; failure is a status and a text, as build_forest reports it.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <thread>

#include "ftte_geometry.h"
#include "ftte_hybrid.h"
#include "ftte_tiles.h"

namespace ftte {

static int fail(std::string *err, int code, const std::string &msg)
{
    if (err) *err = msg;
    return code;
}

// ---- planner ------------------------------------------------------------------------------------
// One direction: fold it (equiSources.f90:1395-1454), build its per-layer patterns (:1495-1534, setPattern) and turn them
// into what the kernels read: the memory frame of its izone and one LayerRec per layer.
int plan_direction(int n_grid, double box, int d, double phi_d, double theta_d, double w_d, int tile_rows, std::vector<ftte_pattern> &pat,
                   std::vector<int> &du_cum, std::vector<int> &dv_cum, DirPlan &D, LayerRec *layers_of_d, size_t layer_off,
                   const SubGridPlan *sub, std::string *err)
{
    // sub: the planes of a cubic sub-grid of `sub->n` cells a side and cell size sub->cell, whose layers carry the patterns
    // sub->patterns(d) instead of a ray's own march from (0.5, 0.5): the fine cells of a fully refined block (ftte_hybrid.cpp)
    const int n = sub ? sub->n : n_grid;
    const double cell = sub ? sub->cell : box / (double)n; // cellSizeAbsoluteUnits, equiSources.f90:1570
    const long nn = (long)n * n;
    D.w = w_d;

    int rc = fold_direction(phi_d, theta_d, &D.phi, &D.theta, &D.izone);
    if (rc) {
        char buf[160];
        std::snprintf(buf, sizeof buf, "direction %d (phi=%.17g, theta=%.17g) cannot be folded: %s", d, phi_d, theta_d,
                      rc == 1 ? "phi on a quadrant boundary" : rc == 2 ? "theta outside (-pi/2,0)u(0,pi/2)"
                                                                       : "tie between dominant axes");
        return fail(err, fold_status(rc), buf);
    }
    if (sub) {
        const int src = sub->patterns(d, D.phi, D.theta, D.izone, pat.data());
        if (src) return fail(err, src, "direction " + std::to_string(d) + ": ray pattern left the unit cell (sub-layer patterns of a refined block)");
    } else if (layer_patterns(n, D.phi, D.theta, pat.data())) {
        char buf[128];
        std::snprintf(buf, sizeof buf, "direction %d: ray pattern left the unit cell (setPattern consistency check)", d);
        return fail(err, FTTE_ERR_PATTERN, buf);
    }

    // memory frame of this izone: which storage axis the march runs along decides the layout;
    // within it u = the sweep axis that lands on the contiguous storage axis
    ZoneMap zm;
    zone_map(D.izone, &zm);
    int march_c = 0;
    for (int a = 0; a < 3; ++a) if (zm.src[a] == 0) march_c = a;
    D.layout = march_c;
    const int fast_c = (march_c == 2) ? 1 : 2;
    const int mid_c = (march_c == 0) ? 1 : 0;
    const bool u_is_k = zm.src[fast_c] == 2;
    D.su = zm.mirror[fast_c] ? -1 : 1;
    D.sv = zm.mirror[mid_c] ? -n : n;
    D.si = (int)(zm.mirror[march_c] ? -nn : nn);
    // the column enters as a position p = u (or n+1-u when mirrored) with stride +1: offset p - 1
    D.org = -1 + (zm.mirror[mid_c] ? (long)n * n : -(long)n) +
            (zm.mirror[march_c] ? (long)n * nn : -nn);

    // layers: reference chain -> kernel-frame class, lengths in chain order, cumulative drift
    D.layer_off = layer_off;
    int du = 0, dv = 0;
    for (int i = 0; i < n; ++i) {
        const ftte_pattern &p = pat[i];
        LayerRec &R = layers_of_d[i];
        R.dpath[0] = cell * p.xy_len;
        R.dpath[1] = R.dpath[2] = 0.0;
        int rc_class = RC_ONE, step_k = 0, step_j = 0;
        if (p.xz_active && p.yz_active) {
            step_k = step_j = 1;
            if (p.xy_top == 3) { // xy -> yz -> xz (the xz piece reaches the top)
                R.dpath[1] = cell * p.yz_len; R.dpath[2] = cell * p.xz_len;
                rc_class = u_is_k ? RC_THREE_U_SWAP : RC_THREE_V_SWAP; // mean adds xy, xz, yz: 3rd piece before 2nd
            } else {             // xy -> xz -> yz
                R.dpath[1] = cell * p.xz_len; R.dpath[2] = cell * p.yz_len;
                rc_class = u_is_k ? RC_THREE_V : RC_THREE_U;
            }
        } else if (p.yz_active) { // xy -> yz: one cell further along sweep-k
            step_k = 1;
            R.dpath[1] = cell * p.yz_len;
            rc_class = u_is_k ? RC_TWO_U : RC_TWO_V;
        } else if (p.xz_active) { // xy -> xz: one cell further along sweep-j
            step_j = 1;
            R.dpath[1] = cell * p.xz_len;
            rc_class = u_is_k ? RC_TWO_V : RC_TWO_U;
        }
        R.info = rc_class;
        R.drift = (du & 0xffff) | (dv << 16);
        du_cum[i] = du; dv_cum[i] = dv;
        du += u_is_k ? step_k : step_j;
        dv += u_is_k ? step_j : step_k;
    }
    // rays present at the last layer start at label -drift (base cell 0, second piece in cell 1)
    D.u_lo = 1 - du_cum[n - 1];
    D.v_lo = 1 - dv_cum[n - 1];
    D.du_mid = du_cum[n / 2];
    D.dv_mid = dv_cum[n / 2];
    D.ntu = (n - D.u_lo + 1 + 62) / 63;
    D.ntv = (n - D.v_lo + 1 + tile_rows - 1) / tile_rows;

    return FTTE_OK;
}

// The part of a brick plan that does not depend on which bricks are swept: the directions, the brick geometry and the face
// block layout, the groups and their accumulators.
int plan_brick_groups(BrickPlan &P, int n_grid, double box, int ndir, const double *phi, const double *theta, const double *w, int chunk, int gmax,
                      int share, int want_dataflow, bool whole_faces, const SubGridPlan *sub, std::string *err)
{
    const int n = sub ? sub->n : n_grid;
    P = BrickPlan();
    P.n = n; P.chunk = chunk;
    P.phi.assign(phi, phi + ndir); P.theta.assign(theta, theta + ndir); P.w.assign(w, w + ndir);
    P.dirs.resize(ndir);
    P.layers.resize((size_t)ndir * n);

    std::vector<ftte_pattern> pat(n);
    std::vector<int> du_cum(n + 1), dv_cum(n + 1);
    for (int d = 0; d < ndir; ++d) {
        const int rc = plan_direction(n_grid, box, d, phi[d], theta[d], w[d], 7, pat, du_cum, dv_cum, P.dirs[d], &P.layers[(size_t)d * n], (size_t)d * n, sub, err);
        if (rc) return rc;
    }
    P.ntu = (n + 63) / 64; P.ntv = (n + kBrickRows - 1) / kBrickRows; P.nti = (n + chunk - 1) / chunk;
    P.up = 64 * P.ntu; P.vp = kBrickRows * P.ntv;
    P.dataflow = want_dataflow != 0;
    P.ut = P.dataflow ? 16 : kBrickRows; // a 128-byte line of its own per brick and layer when bricks of one launch exchange rays
    P.uw = P.ntv * P.ut;
    // rings over two chunks, or every chunk's faces kept (hybrid sweep); a sub-grid keeps one slot more (the chunk before its first)
    // and one ring more along u and v (the brick columns / rows before its first): BrickLaunch::sub
    P.nslot = sub ? P.nti + 1 : whole_faces ? P.nti : 2;
    const int edge = sub ? 1 : 0;
    P.vface_off = (int64_t)(P.ntu + edge) * P.nslot * chunk * P.uw;
    P.iface_off = P.vface_off + (int64_t)(P.ntv + edge) * P.nslot * chunk * P.up;
    P.uqface_off = P.iface_off + (int64_t)P.nslot * P.vp * P.up;
    // (the faces inside a brick are used by the hybrid sweep only, which keeps every chunk's faces)
    P.face_elems = P.uqface_off + (whole_faces ? 2 * (int64_t)P.nslot * chunk * P.uw : 0);

    if (P.nti >= kBrickAccumulate) return fail(err, FTTE_ERR_UNSUPPORTED, "brick engine: more than 16383 chunks along the march axis: raise option \"chunk\"");

    // Groups: layout after layout (the order in which the merge adds the accumulators), izone after izone, at most gmax
    // directions each.  Accumulators: a group stores its J contribution once per cell, and every accumulator costs the merge
    // one more read of the grid, so groups share an accumulator where they provably never meet in a brick in the same launch
    // (the later one then reads, adds and stores, BrickTask):
    //   * the passes of one izone sweep the bricks in the same order: started in different launches they never meet;
    //   * two izones of one layout differ by reflections of the brick order along some axes; with t -> N-1-t along an axis
    //     of even brick count N the difference of their stage numbers in a brick changes by an odd amount, so if an odd number
    //     of such axes is reflected the difference is odd in every brick, and start launches that differ by an even number
    //     never bring them together.  Needs bricks that coincide under reflection: n a multiple of 64, 8 and the chunk.
    const bool aligned = n % 64 == 0 && n % kBrickRows == 0 && n % chunk == 0;
    const int nbricks[3] = {P.ntu, P.ntv, P.nti};
    for (int layout = 0; layout < 3; ++layout) {
        struct Zone { int izone, parity; std::vector<std::vector<int>> passes; };
        std::vector<Zone> zones;
        for (int izone = 1; izone <= 24; ++izone) {
            std::vector<int> members;
            for (int d = 0; d < ndir; ++d)
                if (P.dirs[d].izone == izone && P.dirs[d].layout == layout) members.push_back(d);
            if (members.empty()) continue;
            Zone Z;
            Z.izone = izone;
            const DirPlan &D0 = P.dirs[members[0]];
            const bool mirror[3] = {D0.su < 0, D0.sv < 0, D0.si < 0};
            Z.parity = 0;
            for (int a = 0; a < 3; ++a) if (mirror[a] && nbricks[a] % 2 == 0) Z.parity ^= 1;
            // as few passes as gmax allows, of equal size where possible (5 directions, gmax 4: 3 + 2, not 4 + 1)
            const size_t npass = (members.size() + (size_t)gmax - 1) / (size_t)gmax;
            for (size_t b = 0, q = 0; q < npass; ++q) {
                const size_t len = members.size() / npass + (q < members.size() % npass ? 1 : 0);
                Z.passes.emplace_back(members.begin() + (long)b, members.begin() + (long)(b + len));
                b += len;
            }
            zones.push_back(Z);
        }
        // pair the izones of opposite parity (share = 2); share = 1: only the passes of one izone share; 0: nobody shares
        std::vector<int> partner(zones.size(), -1);
        if (aligned && share >= 2)
            for (size_t x = 0; x < zones.size(); ++x) {
                if (partner[x] >= 0) continue;
                for (size_t y = x + 1; y < zones.size(); ++y)
                    if (partner[y] < 0 && zones[y].parity != zones[x].parity) { partner[x] = (int)y; partner[y] = (int)x; break; }
            }
        std::vector<int> acc_of(zones.size(), -1);
        for (size_t x = 0; x < zones.size(); ++x) {
            const bool paired = partner[x] >= 0;
            if (share >= 1) {
                if (acc_of[x] < 0) {
                    acc_of[x] = P.nacc[layout]++;
                    if (paired) acc_of[(size_t)partner[x]] = acc_of[x];
                }
            }
            for (size_t p = 0; p < zones[x].passes.size(); ++p) {
                BrickPlan::Group G;
                G.izone = zones[x].izone; G.layout = layout;
                G.acc = share >= 1 ? acc_of[x] : P.nacc[layout]++;
                G.offset = share >= 1 ? (int)p * (paired ? 2 : 1) : 0;
                G.dirs = zones[x].passes[p];
                P.max_dirs = std::max(P.max_dirs, (int)G.dirs.size());
                P.groups.push_back(G);
            }
        }
    }
    for (int layout = 0; layout < 3; ++layout)
        if (P.nacc[layout] > kMaxAcc) return fail(err, FTTE_ERR_UNSUPPORTED, "too many direction groups for one memory layout: raise option \"group\"");

    return FTTE_OK;
}

// ---- task lists ------------------------------------------------------------------------------------------------------------------
namespace {

size_t brick_index(const BrickPlan &P, int tu, int tv, int ti) { return ((size_t)ti * P.ntv + tv) * P.ntu + tu; }
// the physical brick under brick (tu, tv, ti) of group G: counted from the far end along the axes the group's frame mirrors
size_t brick_index(const BrickPlan &P, const BrickPlan::Group &G, int tu, int tv, int ti)
{
    const DirPlan &D0 = P.dirs[G.dirs[0]];
    return brick_index(P, D0.su < 0 ? P.ntu - 1 - tu : tu, D0.sv < 0 ? P.ntv - 1 - tv : tv, D0.si < 0 ? P.nti - 1 - ti : ti);
}
template <typename F> void for_each_brick(const BrickPlan &P, F fn)
{
    for (int ti = 0; ti < P.nti; ++ti)
        for (int tv = 0; tv < P.ntv; ++tv)
            for (int tu = 0; tu < P.ntu; ++tu) fn(tu, tv, ti);
}
std::vector<size_t> groups_in_order(const BrickPlan &P)
{
    std::vector<size_t> order(P.groups.size());
    for (size_t g = 0; g < order.size(); ++g) order[g] = g;
    return order;
}
// within a list the groups with the most directions first: their bricks take longest, the short ones fill the tail
std::vector<size_t> largest_groups_first(const BrickPlan &P)
{
    std::vector<size_t> order = groups_in_order(P);
    std::stable_sort(order.begin(), order.end(), [&](size_t x, size_t y) { return P.groups[x].dirs.size() > P.groups[y].dirs.size(); });
    return order;
}

// The one builder of task lists.  visit(g, put) names every task of group g in the order it is to stand in its list:
// put(list, launch, tu, tv, ti, task) -- `list` of the `nlists` it goes into, `launch` the place of that list in the launch order of
// its accumulator's stream, `task` as the kernel reads it but for the accumulate bit.  Counts per list, turns the counts into offsets
// (returned: nlists + 1), fills P.tasks with the groups in `order`, and sets kBrickAccumulate exactly where an earlier launch visits
// the same physical brick of the same accumulator: whoever comes first stores, whoever comes later reads, adds and stores.
// (Two pieces of one brick in one launch write different lanes of rows that start from zero: either may come first.)
template <typename Visit> std::vector<size_t> build_task_lists(BrickPlan &P, const std::vector<size_t> &order, size_t nlists, Visit visit)
{
    const size_t nb = (size_t)P.ntu * P.ntv * P.nti;
    std::vector<std::vector<size_t>> first(3 * (size_t)kMaxAcc); // per accumulator and physical brick: the earliest launch that writes it
    std::vector<size_t> off(nlists + 1, 0);
    for (size_t g : order) {
        const BrickPlan::Group &G = P.groups[g];
        std::vector<size_t> &F = first[(size_t)G.layout * kMaxAcc + G.acc];
        if (F.empty()) F.assign(nb, ~(size_t)0);
        visit(g, [&](size_t list, size_t launch, int tu, int tv, int ti, const BrickTask &) {
            ++off[list + 1];
            size_t &f = F[brick_index(P, G, tu, tv, ti)];
            f = std::min(f, launch);
        });
    }
    for (size_t l = 0; l < nlists; ++l) off[l + 1] += off[l];
    P.tasks.resize(off[nlists]);
    std::vector<size_t> fill(off.begin(), off.end() - 1);
    for (size_t g : order) {
        const BrickPlan::Group &G = P.groups[g];
        const std::vector<size_t> &F = first[(size_t)G.layout * kMaxAcc + G.acc];
        visit(g, [&](size_t list, size_t launch, int tu, int tv, int ti, BrickTask T) {
            if (launch > F[brick_index(P, G, tu, tv, ti)]) T.ti = (int16_t)(T.ti | kBrickAccumulate);
            P.tasks[fill[list]++] = T;
        });
    }
    return off;
}

// ---- the uniform grid's brick plan, step by step ------------------------------------------------------------------------------------

// Streams: the groups of one accumulator stay on one stream (their launches are ordered against each other)
void deal_group_lanes(BrickPlan &P, int want_glanes)
{
    P.glanes = std::max(1, std::min(want_glanes, P.nacc[0] + P.nacc[1] + P.nacc[2]));
    int next = 0;
    std::vector<int> lane_of(3 * (size_t)kMaxAcc, -1);
    for (auto &G : P.groups) {
        int &l = lane_of[(size_t)G.layout * kMaxAcc + G.acc];
        if (l < 0) l = next++ % P.glanes;
        G.lane = l;
    }
}

// Two passes per visit (BrickKey::duo).  The passes of an izone follow each other in P.groups, pass p at stage offset p * step
// (step 2 where the izone is paired with one of opposite parity).  They are linked two by two, (0, 1), (2, 3), ..., an odd last one
// stays alone; visit v = p / 2 takes the place pass v has in a plan of single passes: offset v * step, the izone's accumulator.
// The even pass of a linked visit owns the cells' J, the odd one is its helper.  No izone with two passes: nothing changes.
void link_visits(BrickPlan &P)
{
    const size_t ng = P.groups.size();
    for (size_t g0 = 0, g1; g0 < ng; g0 = g1) {
        for (g1 = g0 + 1; g1 < ng && P.groups[g1].izone == P.groups[g0].izone && P.groups[g1].layout == P.groups[g0].layout; ++g1) {}
        if (g1 - g0 >= 2) P.duo = true;
    }
    P.nvisits = (int)ng;
    if (!P.duo) return;
    P.nvisits = 0;
    for (size_t g0 = 0, g1; g0 < ng; g0 = g1) {
        for (g1 = g0 + 1; g1 < ng && P.groups[g1].izone == P.groups[g0].izone && P.groups[g1].layout == P.groups[g0].layout; ++g1) {}
        const int step = g1 - g0 >= 2 ? P.groups[g0 + 1].offset - P.groups[g0].offset : 1;
        for (size_t g = g0; g < g1; ++g) {
            BrickPlan::Group &G = P.groups[g];
            const size_t p = g - g0;
            G.offset = (int)(p / 2) * step;
            G.helper = p % 2 == 1;
            G.partner = G.helper ? (int)g - 1 : g + 1 < g1 ? (int)g + 1 : -1;
            if (!G.helper) ++P.nvisits;
        }
    }
}

// The seats of every stage list of a plan with two passes per visit: a linked visit's two tasks of a brick in one seat, the owner's
// first; the stage's other tasks two by two in list order (the most directions first), an odd last one with an empty place; then
// the seats with the most directions first.  A helper's task carries no accumulate bit: it neither stores nor reads J.
void seat_stage_lists(BrickPlan &P)
{
    const size_t nb = (size_t)P.ntu * P.ntv * P.nti;
    const size_t none = ~(size_t)0;
    std::vector<size_t> helper_at(P.groups.size() * nb, none); // the helper's task that crosses a brick with its owner's
    for (size_t q = 0; q < P.tasks.size(); ++q) {
        BrickTask &T = P.tasks[q];
        if (!P.groups[(size_t)T.group].helper) continue;
        T.ti = (int16_t)(T.ti & ~kBrickAccumulate);
        helper_at[(size_t)T.group * nb + brick_index(P, T.tu, T.tv, T.ti)] = q;
    }
    auto ndirs = [&](const BrickTask &T) { return T.group < 0 ? (size_t)0 : P.groups[(size_t)T.group].dirs.size(); };
    const BrickTask empty{-1, 0, 0, 0};
    P.seat_off.assign((size_t)P.glanes * ((size_t)P.nstages + 1), 0);
    for (size_t l = 0; l < (size_t)P.glanes; ++l) {
        for (size_t st = 0; st < (size_t)P.nstages; ++st) {
            const size_t q0 = P.stage_off[l * ((size_t)P.nstages + 1) + st], q1 = P.stage_off[l * ((size_t)P.nstages + 1) + st + 1];
            std::vector<BrickSeat> seats;
            std::vector<BrickTask> lone;
            for (size_t q = q0; q < q1; ++q) {
                const BrickTask &T = P.tasks[q];
                const BrickPlan::Group &G = P.groups[(size_t)T.group];
                if (G.helper) continue;
                if (G.partner < 0) { lone.push_back(T); continue; }
                BrickTask own = T, help = P.tasks[helper_at[(size_t)G.partner * nb + brick_index(P, T.tu, T.tv, T.ti & (kBrickAccumulate - 1))]];
                own.ti = (int16_t)(own.ti | kBrickLinked); help.ti = (int16_t)(help.ti | kBrickLinked);
                seats.push_back(BrickSeat{{own, help}});
                ++P.nlinked;
            }
            for (size_t k = 0; k < lone.size(); k += 2) seats.push_back(BrickSeat{{lone[k], k + 1 < lone.size() ? lone[k + 1] : empty}});
            std::stable_sort(seats.begin(), seats.end(), [&](const BrickSeat &x, const BrickSeat &y) { return ndirs(x.place[0]) + ndirs(x.place[1]) > ndirs(y.place[0]) + ndirs(y.place[1]); });
            P.seats.insert(P.seats.end(), seats.begin(), seats.end());
            P.seat_off[l * ((size_t)P.nstages + 1) + st + 1] = P.seats.size();
        }
        if (l + 1 < (size_t)P.glanes) P.seat_off[(l + 1) * ((size_t)P.nstages + 1)] = P.seats.size();
    }
}

// Stages: brick (tu, tv, ti) of a group runs in stage tu + tv + ti + the group's offset of its lane.  Fills P.tasks, P.nstages,
// P.stage_off ([glanes][nstages + 1], the lanes one after the other) and P.updates.
void write_stage_lists(BrickPlan &P, int ndir)
{
    int max_offset = 0;
    for (const auto &G : P.groups) max_offset = std::max(max_offset, G.offset);
    const size_t nstages = P.groups.empty() ? 0 : (size_t)(P.ntu + P.ntv + P.nti - 2 + max_offset);
    P.nstages = (int)nstages;
    const std::vector<size_t> off = build_task_lists(P, largest_groups_first(P), (size_t)P.glanes * nstages, [&](size_t g, auto put) {
        const BrickPlan::Group &G = P.groups[g];
        for_each_brick(P, [&](int tu, int tv, int ti) {
            const size_t st = (size_t)(tu + tv + ti + G.offset);
            put((size_t)G.lane * nstages + st, st, tu, tv, ti, BrickTask{(int16_t)g, (int16_t)tu, (int16_t)tv, (int16_t)ti});
        });
    });
    P.stage_off.resize((size_t)P.glanes * (nstages + 1));
    for (size_t l = 0; l < (size_t)P.glanes; ++l)
        for (size_t st = 0; st <= nstages; ++st) P.stage_off[l * (nstages + 1) + st] = off[l * nstages + st];
    P.updates = (int64_t)P.n * P.n * P.n * ndir; // (every group's bricks cover the grid)
}

// One-launch forms: what each brick waits for -- its three upstream neighbours, the readers of the two face slots it rewrites (the
// rings hold two chunks), and the previous visitor of its J tile.  All of them lie earlier in the (stage-ordered) list.
int link_dependencies(BrickPlan &P, std::string *err)
{
    const size_t nt = P.tasks.size(), nb = (size_t)P.ntu * P.ntv * P.nti;
    std::vector<int32_t> index(P.groups.size() * nb, -1);
    auto at = [&](size_t g, int tu, int tv, int ti) -> int32_t & { return index[g * nb + brick_index(P, tu, tv, ti)]; };
    for (size_t q = 0; q < nt; ++q) at((size_t)P.tasks[q].group, P.tasks[q].tu, P.tasks[q].tv, P.tasks[q].ti & (kBrickAccumulate - 1)) = (int32_t)q;
    P.deps.assign(nt * kBrickDeps, -1);
    // the visitors of every J tile, per accumulator, in launch order
    struct Visit { int launch; int32_t task; };
    std::vector<std::vector<std::vector<Visit>>> visits(3 * (size_t)kMaxAcc);
    for (size_t q = 0; q < nt; ++q) {
        const BrickTask &T = P.tasks[q];
        const size_t g = (size_t)T.group;
        const BrickPlan::Group &G = P.groups[g];
        const int ti = T.ti & (kBrickAccumulate - 1);
        int32_t *D = &P.deps[q * kBrickDeps];
        if (T.tu > 0) D[0] = at(g, T.tu - 1, T.tv, ti);
        if (T.tv > 0) D[1] = at(g, T.tu, T.tv - 1, ti);
        if (ti > 0) D[2] = at(g, T.tu, T.tv, ti - 1);
        if (ti >= 2 && T.tu + 1 < P.ntu) D[4] = at(g, T.tu + 1, T.tv, ti - 2); // read the u-face slot this brick rewrites
        if (ti >= 2 && T.tv + 1 < P.ntv) D[5] = at(g, T.tu, T.tv + 1, ti - 2); // the v-face slot
        auto &V = visits[(size_t)G.layout * kMaxAcc + G.acc];
        if (V.empty()) V.resize(nb);
        V[brick_index(P, G, T.tu, T.tv, ti)].push_back({T.tu + T.tv + ti + G.offset, (int32_t)q});
    }
    for (auto &V : visits)
        for (auto &list : V) {
            std::sort(list.begin(), list.end(), [](const Visit &x, const Visit &y) { return x.launch < y.launch; });
            for (size_t k = 1; k < list.size(); ++k) P.deps[(size_t)list[k].task * kBrickDeps + 3] = list[k - 1].task;
        }
    for (size_t q = 0; q < nt; ++q)
        for (int k = 0; k < kBrickDeps; ++k)
            if (P.deps[q * kBrickDeps + k] >= (int32_t)q) return fail(err, FTTE_ERR_STATE, "brick plan: a dependency does not precede its brick");
    return FTTE_OK;
}

// Merge blocks: the stage of the last task that writes into each kMergeBlock^3 block of cells, in any accumulator.  A brick holds,
// along the storage axes (ic, jc, kc) of its layout, the layers chunk * ti + 1 .. of the march axis, the rows kBrickRows * tv + 1 ..
// of the middle one and the columns 64 tu + 1 .. of the contiguous one, each counted from the far end where the frame mirrors it.
// The blocks are then cut into merge points: after the stages by which half, three quarters, ... of them are final, and after the
// last stage.  (Points from an eighth of the blocks on: 0.3 ms per 256^3 x 8 x 96 step slower -- the early merges only take
// bandwidth from wide stages -- and three points: 0.1 ms slower; profiles/README.md.)
void cut_merge_points(BrickPlan &P)
{
    const int n = P.n, nstages = P.nstages, nmb = (n + kMergeBlock - 1) / kMergeBlock;
    const size_t nblk = (size_t)nmb * nmb * nmb;
    P.nmb = nmb;
    std::vector<int> last(nblk, nstages - 1); // (every block is written; the default only keeps a gap safe)
    std::vector<char> seen(nblk, 0);
    for (int st = 0; st < nstages; ++st)
        for (size_t q = P.stage_off[(size_t)st]; q < P.stage_off[(size_t)st + 1]; ++q) {
            const BrickTask &T = P.tasks[q];
            const BrickPlan::Group &G = P.groups[(size_t)T.group];
            const DirPlan &D0 = P.dirs[G.dirs[0]];
            const int march_c = G.layout, fast_c = march_c == 2 ? 1 : 2, mid_c = march_c == 0 ? 1 : 0;
            int lo[3], hi[3];
            auto span = [&](int axis, int first, int len, bool mirror) { // cells first .. first + len - 1 (0-based) of the frame axis
                const int a = first, b = std::min(first + len, n) - 1;
                lo[axis] = (mirror ? n - 1 - b : a) / kMergeBlock;
                hi[axis] = (mirror ? n - 1 - a : b) / kMergeBlock;
            };
            span(march_c, P.chunk * (T.ti & (kBrickAccumulate - 1)), P.chunk, D0.si < 0);
            span(mid_c, kBrickRows * T.tv, kBrickRows, D0.sv < 0);
            span(fast_c, 64 * T.tu, 64, D0.su < 0);
            for (int bi = lo[0]; bi <= hi[0]; ++bi)
                for (int bj = lo[1]; bj <= hi[1]; ++bj)
                    for (int bk = lo[2]; bk <= hi[2]; ++bk) {
                        const size_t b = ((size_t)bi * nmb + bj) * nmb + bk;
                        last[b] = seen[b] ? std::max(last[b], st) : st;
                        seen[b] = 1;
                    }
        }
    std::vector<int32_t> order(nblk);
    for (size_t b = 0; b < nblk; ++b) order[b] = (int32_t)b;
    std::stable_sort(order.begin(), order.end(), [&](int32_t x, int32_t y) { return last[(size_t)x] < last[(size_t)y]; });
    static const double kFrac[] = {4. / 8, 6. / 8, 7. / 8, 15. / 16, 31. / 32, 1.};
    P.merge_off.push_back(0);
    for (double f : kFrac) {
        const size_t want = std::min(nblk, std::max<size_t>(1, (size_t)std::ceil(f * (double)nblk)));
        const int st = f >= 1. ? nstages - 1 : last[(size_t)order[want - 1]];
        if (!P.merge_stage.empty() && st <= P.merge_stage.back()) continue;
        size_t end = P.merge_off.back();
        while (end < nblk && last[(size_t)order[end]] <= st) ++end;
        if (end == P.merge_off.back() && st != nstages - 1) continue;
        P.merge_stage.push_back(st);
        P.merge_off.push_back(end);
    }
    P.merge_blocks = std::move(order);
}

// Queues of the persistent form.  What a brick waits for belongs to its own frequency group and to the groups of directions that share
// its accumulator, so (frequency group, accumulator) pairs are the units that can be dealt out.  With a multiple of the queue count
// in frequency groups, queue = group mod queues (all direction groups of a frequency group read the same opacities: one L2 for them);
// else the units go, largest first, to the queue with the least work so far.
void deal_queues(BrickPlan &P, int nnu, int nq, int queue_mix)
{
    const int64_t n = P.n;
    P.persistent = true;
    std::vector<int64_t> acc_dirs(3 * (size_t)kMaxAcc, 0);
    for (const auto &G : P.groups) acc_dirs[(size_t)G.layout * kMaxAcc + G.acc] += (int64_t)G.dirs.size();
    std::vector<int> queue_of((size_t)nnu * 3 * kMaxAcc, -1);
    int64_t load[kBrickQueues] = {};
    if (nnu % nq == 0 && queue_mix == 0) {
        for (int nu = 0; nu < nnu; ++nu)
            for (size_t a = 0; a < acc_dirs.size(); ++a)
                if (acc_dirs[a]) { queue_of[(size_t)nu * acc_dirs.size() + a] = nu % nq; load[nu % nq] += acc_dirs[a]; }
    } else if (queue_mix == 2) { // every queue a share of every frequency group: accumulator a of group nu to queue (nu + a) mod queues
        for (int nu = 0; nu < nnu; ++nu) {
            int k = 0;
            for (size_t a = 0; a < acc_dirs.size(); ++a)
                if (acc_dirs[a]) { const int q = (nu + k++) % nq; queue_of[(size_t)nu * acc_dirs.size() + a] = q; load[q] += acc_dirs[a]; }
        }
    } else {
        std::vector<std::pair<int64_t, size_t>> units;
        for (int nu = 0; nu < nnu; ++nu)
            for (size_t a = 0; a < acc_dirs.size(); ++a)
                if (acc_dirs[a]) units.push_back({acc_dirs[a], (size_t)nu * acc_dirs.size() + a});
        std::stable_sort(units.begin(), units.end(), [](const auto &x, const auto &y) { return x.first > y.first; });
        for (const auto &u : units) {
            int q = 0;
            for (int k = 1; k < nq; ++k) if (load[k] < load[q]) q = k;
            queue_of[u.second] = q;
            load[q] += u.first;
        }
    }
    std::vector<std::vector<uint32_t>> lists((size_t)nq);
    for (size_t t = 0; t < P.tasks.size(); ++t) {
        const BrickPlan::Group &G = P.groups[(size_t)P.tasks[t].group];
        const size_t a = (size_t)G.layout * kMaxAcc + G.acc;
        for (int nu = 0; nu < nnu; ++nu)
            lists[(size_t)queue_of[(size_t)nu * acc_dirs.size() + a]].push_back((uint32_t)(t * (size_t)nnu + (size_t)nu));
    }
    for (int q = 0; q < kBrickQueues; ++q) {
        P.qoff[q] = (uint32_t)P.queue.size();
        P.qlen[q] = q < nq ? (uint32_t)lists[(size_t)q].size() : 0;
        P.qload[q] = q < nq ? load[q] * n * n * n : 0;
        if (q < nq) P.queue.insert(P.queue.end(), lists[(size_t)q].begin(), lists[(size_t)q].end());
    }
}

} // namespace

// Bricks: group the directions by izone (input order within an izone, at most gmax per group), cut the grid into bricks of
// 64 x kBrickRows x chunk cells, and order the bricks of every group into stages tu + tv + ti: a brick's three upstream neighbours
// lie one stage earlier, its consumers exactly one stage later (which is what lets the face buffers be rings over two chunks).
int plan_bricks(const BrickInputs &in, BrickPlan &P, std::string *err)
{
    const BrickKey &K = in.key;
    int rc;
    if ((rc = plan_brick_groups(P, K.n, K.box, in.ndir, in.phi, in.theta, in.w, K.chunk, K.gmax, K.share, K.want_dataflow, false, nullptr, err))) return rc;
    P.key = K;
    P.nvisits = (int)P.groups.size();
    if (K.duo) link_visits(P);
    deal_group_lanes(P, K.want_glanes);
    write_stage_lists(P, in.ndir);
    if (P.duo) seat_stage_lists(P);
    if (P.dataflow && !P.tasks.empty() && (rc = link_dependencies(P, err))) return rc;
    if (!P.dataflow && P.glanes == 1 && !P.tasks.empty()) cut_merge_points(P); // (merge points: stages on one lane of groups)
    if (P.dataflow && K.want_dataflow == 3 && !P.tasks.empty()) deal_queues(P, K.nnu, K.xcc_count, K.queue_mix);
    P.valid = true;
    return FTTE_OK;
}

// Ray-following tiles: turns the direction list into what the tile kernel consumes.  O(ndir * (n + tiles)) host work.
int plan_tiles(const TileInputs &in, Plan &P, std::string *err)
{
    const int n = in.n, slots = in.slots, ndir = in.ndir;
    const int tile_rows = in.stack * in.rows - 1; // owned rows of one work item
    P = Plan();
    P.n = n; P.rows = in.rows; P.slots = slots; P.stack = in.stack; P.box = in.box;
    P.phi.assign(in.phi, in.phi + ndir); P.theta.assign(in.theta, in.theta + ndir); P.w.assign(in.w, in.w + ndir);
    P.dirs.resize(ndir);
    P.layers.resize((size_t)ndir * n);

    std::vector<ftte_pattern> pat(n);
    std::vector<int> du_cum(n + 1), dv_cum(n + 1);
    int in_layout[3] = {0, 0, 0};

    for (int d = 0; d < ndir; ++d) {
        DirPlan &D = P.dirs[d];
        const int rc = plan_direction(n, in.box, d, in.phi[d], in.theta[d], in.w[d], tile_rows, pat, du_cum, dv_cum, D, &P.layers[(size_t)d * n], (size_t)d * n, nullptr, err);
        if (rc) return rc;
        D.slot = in_layout[D.layout]++ % slots;
    }

    // launches: per layout, batches of `slots` directions in input order
    for (int layout = 0; layout < 3; ++layout) {
        std::vector<int> members;
        for (int d = 0; d < ndir; ++d) if (P.dirs[d].layout == layout) members.push_back(d);
        for (size_t b = 0; b < members.size(); b += slots) {
            LaunchPlan LP;
            LP.layout = layout;
            LP.first = (b == 0);
            // a short last batch takes the highest accumulators: the lower ones are final one launch earlier and can be
            // merged while it runs, without changing the order in which the accumulators are added up
            const int in_batch = (int)(std::min(members.size(), b + (size_t)slots) - b);
            LP.acc_base = (b > 0 && in_batch < slots) ? slots - in_batch : 0;
            LP.item_off = P.items.size();
            std::vector<uint32_t> where; // per item of this launch: the tile's place in the plane halfway through the march
            for (size_t s = b; s < std::min(members.size(), b + (size_t)slots); ++s) {
                const int d = members[s];
                const DirPlan &D = P.dirs[d];
                const int slot = (int)(s - b);
                LP.dirs.push_back(d);
                P.used[layout][LP.acc_base + slot] = true;
                const LayerRec *Ls = &P.layers[D.layer_off];
                for (int tv = 0; tv < D.ntv; ++tv) {
                    for (int tu = 0; tu < D.ntu; ++tu) {
                        // owned labels of this tile; a layer is active when any owned ray, or the cell one
                        // step beyond it, is inside the domain
                        const int ul_min = D.u_lo + 63 * tu, ul_max = ul_min + 62;
                        const int vl_min = D.v_lo + tile_rows * tv, vl_max = vl_min + tile_rows - 1;
                        int i_first = 0, i_last = -1;
                        for (int i = 1; i <= n; ++i) {
                            const int cu_d = (int)(short)(Ls[i - 1].drift & 0xffff), cv_d = Ls[i - 1].drift >> 16;
                            const bool act = ul_min + cu_d <= n && ul_max + cu_d + 1 >= 1 && vl_min + cv_d <= n &&
                                             vl_max + cv_d + 1 >= 1;
                            if (act) { if (!i_first) i_first = i; i_last = i; }
                        }
                        if (!i_first) continue;
                        WorkItem it;
                        it.slot = (int16_t)slot; it.tu = (int16_t)tu; it.tv = (int16_t)tv;
                        it.i_first = (int16_t)i_first; it.i_last = (int16_t)i_last; it.pad = 0;
                        P.items.push_back(it);
                        const int pu = std::max(0, ul_min + D.du_mid + 64) / 64, pv = std::max(0, vl_min + D.dv_mid + 64) / std::max(tile_rows, 1);
                        where.push_back(((uint32_t)pv << 16) | (uint32_t)(pu & 0xffff));
                    }
                }
                LP.updates += (int64_t)n * n * n;
            }
            LP.nitems = (int)(P.items.size() - LP.item_off);
            // longest marches first, so that the short corner tiles fill the tail of the launch; among equally long ones, tiles
            // of the directions in flight that cross the same part of the grid side by side, so that they read the same part of
            // a kappa plane at about the same time (+2 %; the place is taken halfway through the march).  (Grouping the tiles of
            // one direction together instead -- hoping for L2 hits on shared halo rows -- was measured: no drop in FETCH_SIZE,
            // 6 % slower through worse load balance.)
            std::vector<uint32_t> idx(where.size());
            for (size_t q = 0; q < idx.size(); ++q) idx[q] = (uint32_t)q;
            const WorkItem *base = P.items.data() + LP.item_off;
            std::stable_sort(idx.begin(), idx.end(), [&](uint32_t x, uint32_t y) {
                const int lx = base[x].i_last - base[x].i_first, ly = base[y].i_last - base[y].i_first;
                if (lx != ly) return lx > ly;
                if (where[x] != where[y]) return where[x] < where[y];
                return base[x].slot < base[y].slot;
            });
            std::vector<WorkItem> sorted(idx.size());
            for (size_t q = 0; q < idx.size(); ++q) sorted[q] = base[idx[q]];
            std::copy(sorted.begin(), sorted.end(), P.items.begin() + LP.item_off);
            P.launches.push_back(LP);
        }
    }
    P.valid = true;
    return FTTE_OK;
}

namespace {

// Where the refined base cells are, in storage coordinates (1-based, inclusive): one bounding box per cluster.  Two refined cells
// belong to one cluster when they lie within two 8-cell blocks of each other; what the per-izone alignment below still brings
// into contact is merged there.
struct Extent { int lo[3], hi[3]; };

std::vector<Extent> refined_clusters(const AmrTree &T)
{
    const int n = T.n, M = 8, nm = (n + M - 1) / M;
    std::vector<int32_t> label((size_t)nm * nm * nm, -2); // -2: no refined cell, -1: not yet labelled
    for (int64_t b = 0; b < (int64_t)n * n * n; ++b)
        if (T.child0[(size_t)b] >= 0)
            label[(((size_t)(b / ((int64_t)n * n)) / M) * nm + (size_t)((b / n) % n) / M) * nm + (size_t)(b % n) / M] = -1;
    int32_t count = 0;
    std::vector<int32_t> stack;
    for (int32_t m0 = 0; m0 < (int32_t)label.size(); ++m0) {
        if (label[(size_t)m0] != -1) continue;
        label[(size_t)m0] = count;
        stack.assign(1, m0);
        while (!stack.empty()) {
            const int32_t m = stack.back();
            stack.pop_back();
            const int a = m / (nm * nm), b = (m / nm) % nm, c2 = m % nm;
            for (int da = -2; da <= 2; ++da)
                for (int db = -2; db <= 2; ++db)
                    for (int dc = -2; dc <= 2; ++dc) {
                        const int x = a + da, y = b + db, z = c2 + dc;
                        if (x < 0 || y < 0 || z < 0 || x >= nm || y >= nm || z >= nm) continue;
                        int32_t &l = label[((size_t)x * nm + y) * nm + z];
                        if (l == -1) { l = count; stack.push_back((int32_t)(((size_t)x * nm + y) * nm + z)); }
                    }
        }
        ++count;
    }
    std::vector<Extent> out((size_t)count);
    for (auto &e : out) for (int a = 0; a < 3; ++a) { e.lo[a] = n + 1; e.hi[a] = 0; }
    for (int64_t b = 0; b < (int64_t)n * n * n; ++b)
        if (T.child0[(size_t)b] >= 0) {
            const int cc[3] = {(int)(b / ((int64_t)n * n)) + 1, (int)((b / n) % n) + 1, (int)(b % n) + 1};
            Extent &e = out[(size_t)label[(((size_t)(cc[0] - 1) / M) * nm + (size_t)(cc[1] - 1) / M) * nm + (size_t)(cc[2] - 1) / M]];
            for (int a = 0; a < 3; ++a) { e.lo[a] = std::min(e.lo[a], cc[a]); e.hi[a] = std::max(e.hi[a], cc[a]); }
        }
    return out;
}

// A box of one izone: the refined cells of a cluster (`fine`: their extent in the sweep frame i, j, k) and a rim of unrefined ones,
// on brick boundaries along v and the march axis (one brick of rim) and, along u, one cell of rim (option "box_lanes": then outwards
// to the next multiple of it): a brick is 64 lanes wide, and whole bricks of rim would put every column of a 128^3 grid into the box
// of a 32^3 patch.  Bricks that a box cuts through sweep the lanes outside it (brick_kernel<..., MASKED>).
struct HybridBox {
    Extent fine;        // sweep frame
    ForestRegion R;
    int lo[3], hi[3];   // the bricks the box touches: u, v, march axis
    int ulo, uhi;       // its cells along u
    int level = 0;      // pass of its forest: 1 + the highest level among the boxes it lies behind
};

void align_box(int n, int lanes, const BrickPlan &P, bool u_is_k, HybridBox *B)
{
    const int ju = u_is_k ? 2 : 1, jv = u_is_k ? 1 : 2; // sweep axes of u and v
    const int *slo = B->fine.lo, *shi = B->fine.hi;
    const int tsize_i = P.chunk, tsize_u = 64, tsize_v = kBrickRows;
    // lanes (option "box_lanes"): 1 (the rim and no more), a multiple such as 16, or 64: whole bricks along u as along the other axes
    B->ulo = lanes == 64 ? std::max(0, (slo[ju] - 1) / 64 - 1) * 64 + 1 : std::max(0, (slo[ju] - 2) / lanes) * lanes + 1;
    B->uhi = lanes == 64 ? std::min(n, (std::min(P.ntu - 1, (shi[ju] - 1) / 64 + 1) + 1) * 64) : std::min(n, (shi[ju] + lanes) / lanes * lanes);
    B->lo[0] = (B->ulo - 1) / tsize_u; B->hi[0] = (B->uhi - 1) / tsize_u;
    B->lo[1] = std::max(0, (slo[jv] - 1) / tsize_v - 1); B->hi[1] = std::min(P.ntv - 1, (shi[jv] - 1) / tsize_v + 1);
    B->lo[2] = std::max(0, (slo[0] - 1) / tsize_i - 1);  B->hi[2] = std::min(P.nti - 1, (shi[0] - 1) / tsize_i + 1);
    ForestRegion *R = &B->R;
    R->u_is_k = u_is_k;
    R->lo[0] = B->lo[2] * tsize_i + 1; R->hi[0] = std::min(n, (B->hi[2] + 1) * tsize_i);
    R->lo[ju] = B->ulo; R->hi[ju] = B->uhi;
    R->lo[jv] = B->lo[1] * tsize_v + 1; R->hi[jv] = std::min(n, (B->hi[1] + 1) * tsize_v);
    R->chunk = P.chunk; R->ut = P.ut; R->nslot = P.nslot; R->ntv = P.ntv; R->up = P.up; R->vp = P.vp;
    R->vface_off = P.vface_off; R->iface_off = P.iface_off; R->uqface_off = P.uqface_off;
}

// The boxes of one izone: every cluster's, merged where two would touch or cut through the same brick, with their levels: box B lies
// behind box A when some ray can pass A first and B later (B's last brick >= A's first one on every axis).  Then B's forest needs the
// bricks in between, which need A's: A is swept in an earlier pass.
std::vector<HybridBox> izone_boxes(int n, int lanes, const BrickPlan &P, int izone, const std::vector<Extent> &clusters)
{
    ZoneMap zm;
    zone_map(izone, &zm);
    int march_c = 0;
    for (int a = 0; a < 3; ++a) if (zm.src[a] == 0) march_c = a;
    const int fast_c = (march_c == 2) ? 1 : 2;
    const bool u_is_k = zm.src[fast_c] == 2;
    std::vector<HybridBox> boxes;
    for (const Extent &e : clusters) {
        HybridBox B;
        for (int a = 0; a < 3; ++a) {
            const int sa = zm.src[a];
            B.fine.lo[sa] = zm.mirror[a] ? n + 1 - e.hi[a] : e.lo[a];
            B.fine.hi[sa] = zm.mirror[a] ? n + 1 - e.lo[a] : e.hi[a];
        }
        align_box(n, lanes, P, u_is_k, &B);
        boxes.push_back(B);
    }
    auto join = [&](size_t x, size_t y) {
        for (int a = 0; a < 3; ++a) {
            boxes[x].fine.lo[a] = std::min(boxes[x].fine.lo[a], boxes[y].fine.lo[a]);
            boxes[x].fine.hi[a] = std::max(boxes[x].fine.hi[a], boxes[y].fine.hi[a]);
        }
        align_box(n, lanes, P, u_is_k, &boxes[x]);
        boxes.erase(boxes.begin() + (long)y);
    };
    for (bool changed = true; changed;) {
        changed = false;
        for (size_t x = 0; x < boxes.size() && !changed; ++x)
            for (size_t y = x + 1; y < boxes.size() && !changed; ++y) {
                const HybridBox &A = boxes[x], &B = boxes[y];
                // too close: next to each other brick-wise along v and the march axis and, along u, in one brick or within two cells
                const bool near_v = A.lo[1] - 1 <= B.hi[1] && B.lo[1] - 1 <= A.hi[1], near_i = A.lo[2] - 1 <= B.hi[2] && B.lo[2] - 1 <= A.hi[2];
                const bool near_u = (A.lo[0] <= B.hi[0] && B.lo[0] <= A.hi[0]) || (A.ulo - 2 <= B.uhi && B.ulo - 2 <= A.uhi);
                // each behind the other: cannot be ordered
                bool a_then_b = true, b_then_a = true;
                for (int k = 0; k < 3; ++k) { a_then_b = a_then_b && B.hi[k] >= A.lo[k]; b_then_a = b_then_a && A.hi[k] >= B.lo[k]; }
                if ((near_u && near_v && near_i) || (a_then_b && b_then_a)) { join(x, y); changed = true; }
            }
    }
    // levels: longest chain of boxes in front.  The relation has no cycles among boxes that do not intersect; should the relaxation
    // not settle all the same, one box takes everything.
    const size_t K = boxes.size();
    bool settled = false;
    for (size_t round = 0; round <= K && !settled; ++round) {
        settled = true;
        for (size_t y = 0; y < K; ++y)
            for (size_t x = 0; x < K; ++x) {
                if (x == y) continue;
                bool x_then_y = true;
                for (int k = 0; k < 3; ++k) x_then_y = x_then_y && boxes[y].hi[k] >= boxes[x].lo[k];
                if (x_then_y && boxes[y].level < boxes[x].level + 1) { boxes[y].level = boxes[x].level + 1; settled = false; }
            }
    }
    if (!settled) {
        while (boxes.size() > 1) join(0, 1);
        boxes[0].level = 0;
    }
    for (size_t x = 0; x < boxes.size(); ++x) { boxes[x].R.id = (int)x; boxes[x].R.pass = boxes[x].level; }
    return boxes;
}

} // namespace

// ---- the hybrid planner, step by step ------------------------------------------------------------------------------------------
namespace {

using Boxes = std::vector<std::vector<HybridBox>>; // per group of directions

// The boxes of every group; is the part outside them worth a brick sweep?  (H: worthwhile, npass, most_boxes; P: the face block
// with every box's own pair of face rings for rays that cross its u-faces inside a brick.)
Boxes boxes_of_groups(int n, int lanes, BrickPlan &P, const std::vector<Extent> &clusters, HybridPlan &H)
{
    Boxes boxes(P.groups.size());
    int64_t inside_bricks = 0, all_bricks = 0;
    int most_boxes = 0, top_level = 0;
    for (size_t g = 0; g < P.groups.size(); ++g) {
        if (g > 0 && P.groups[g].izone == P.groups[g - 1].izone) boxes[g] = boxes[g - 1];
        else boxes[g] = izone_boxes(n, lanes, P, P.groups[g].izone, clusters);
        all_bricks += (int64_t)P.ntu * P.ntv * P.nti;
        most_boxes = std::max(most_boxes, (int)boxes[g].size());
        for (const HybridBox &B : boxes[g]) {
            inside_bricks += (int64_t)(B.hi[0] - B.lo[0] + 1) * (B.hi[1] - B.lo[1] + 1) * (B.hi[2] - B.lo[2] + 1);
            top_level = std::max(top_level, B.level);
        }
    }
    P.face_elems = P.uqface_off + 2 * (int64_t)std::max(most_boxes, 1) * P.nslot * P.chunk * P.uw;
    H.worthwhile = !P.groups.empty() && most_boxes > 0 && most_boxes <= kBrickBoxMask && inside_bricks * 2 <= all_bricks; // else: the forest path for the whole tree
    H.npass = top_level + 1;
    H.most_boxes = most_boxes;
    return boxes;
}

// Several passes: every brick gets the earliest launch its own inputs allow ("slots", assign_slots) instead of a phase per pass,
// which needs accumulators that are not shared between groups (the proof that two groups of one accumulator never meet in a
// launch rests on launch = stage + offset).  36 accumulators of a 128^3 base grid are 5 GB and 1 ms of merge.
// Returns whether the lists go by slot; then every group of P has an accumulator of its own.
bool slot_form(const HybridOptions &opt, int ndir, int npass, BrickPlan &P)
{
    bool slots = (npass > 1 && opt.slots) || opt.slots == 2;
    // Forest batches smaller than the direction list (option "forest_batch") put all pipelines' forests into one run on one stream,
    // which has ONE place in the launch sequence: only the phase form gives every pipeline the same place for a pass.  (Where it is
    // the device memory that makes the batch small, hybrid_sweep finds out later and leaves such a sweep to the forest path.)
    if (opt.forest_batch > 0 && opt.forest_batch < ndir) slots = false;
    if (slots) {
        int per_layout[3] = {0, 0, 0};
        for (const auto &G : P.groups) ++per_layout[G.layout];
        if (per_layout[0] > kMaxAcc || per_layout[1] > kMaxAcc || per_layout[2] > kMaxAcc) slots = false;
    }
    if (slots) {
        P.nacc[0] = P.nacc[1] = P.nacc[2] = 0;
        for (auto &G : P.groups) { G.acc = P.nacc[G.layout]++; G.offset = 0; }
    }
    return slots;
}

// Pipelines ("halves" in the names): the forests stream records at the memory system's rate while the brick stages of a
// 128^3 grid are short launches that leave most of it idle, so the sweep runs as up to four independent sequences (bricks -
// forests - bricks ...) on streams of their own.  What the groups of one accumulator write is ordered by their launches, so
// an accumulator's groups stay together; the pipelines are balanced by direction count.
// Returns the pipeline of every group; *half_dirs: the directions of each pipeline, list order.
std::vector<int> deal_pipelines(const BrickPlan &P, int pipelines, int ndir, std::vector<std::vector<int>> *half_dirs)
{
    std::vector<int> half_of_group(P.groups.size(), 0);
    int nhalves = 1;
    if (pipelines > 1 && P.nacc[0] + P.nacc[1] + P.nacc[2] >= 2) {
        nhalves = std::min(pipelines, P.nacc[0] + P.nacc[1] + P.nacc[2]);
        std::vector<int> weight(3 * (size_t)kMaxAcc, 0), order;
        for (const auto &G : P.groups) weight[(size_t)G.layout * kMaxAcc + G.acc] += (int)G.dirs.size();
        for (int a = 0; a < 3 * kMaxAcc; ++a) if (weight[(size_t)a]) order.push_back(a);
        std::stable_sort(order.begin(), order.end(), [&](int x, int y) { return weight[(size_t)x] > weight[(size_t)y]; });
        std::vector<int> half_of_acc(3 * (size_t)kMaxAcc, 0);
        int load[kMaxPipes] = {0, 0, 0, 0};
        for (int a : order) {
            int h = 0;
            for (int q = 1; q < nhalves; ++q) if (load[q] < load[h]) h = q;
            half_of_acc[(size_t)a] = h; load[h] += weight[(size_t)a];
        }
        for (size_t g = 0; g < P.groups.size(); ++g) half_of_group[g] = half_of_acc[(size_t)P.groups[g].layout * kMaxAcc + P.groups[g].acc];
    }
    half_dirs->assign((size_t)nhalves, std::vector<int>());
    std::vector<int> half_of_dir((size_t)ndir, 0);
    for (size_t g = 0; g < P.groups.size(); ++g) for (int d : P.groups[g].dirs) half_of_dir[(size_t)d] = half_of_group[g];
    for (int d = 0; d < ndir; ++d) (*half_dirs)[(size_t)half_of_dir[(size_t)d]].push_back(d);
    return half_of_group;
}

// ---- a fully refined block swept by bricks of its own on the fine level.  One cluster, a cube of q base cells a side refined
// exactly once, 2 q a multiple of the bricks' 64 lanes and of fine_chunk; `allowed`: the option, one pass, launch lists by phase.
// Returns the block (active, n, lo), or one that is not active.
HybridPlan::Fine fine_block_of(const AmrTree &tree, const std::vector<Extent> &clusters, bool allowed, int fine_chunk)
{
    HybridPlan::Fine FN;
    if (!allowed || clusters.size() != 1) return FN;
    const int n = tree.n;
    const Extent &e = clusters[0];
    const int q = e.hi[0] - e.lo[0] + 1;
    bool cube = q == e.hi[1] - e.lo[1] + 1 && q == e.hi[2] - e.lo[2] + 1 && (2 * q) % 64 == 0 && (2 * q) % fine_chunk == 0 && 2 * q <= 32000;
    for (int a = e.lo[0]; a <= e.hi[0] && cube; ++a)
        for (int b = e.lo[1]; b <= e.hi[1] && cube; ++b)
            for (int d = e.lo[2]; d <= e.hi[2] && cube; ++d) {
                const int32_t node = (int32_t)(((int64_t)(a - 1) * n + (b - 1)) * n + (d - 1));
                const int32_t c0 = tree.child0[(size_t)node];
                if (c0 < 0) { cube = false; break; }
                for (int k = 0; k < 8; ++k) if (tree.child0[(size_t)(c0 + k)] >= 0) cube = false; // refined once, no deeper
            }
    if (cube) {
        FN.active = true;
        FN.n = 2 * q;
        for (int a = 0; a < 3; ++a) FN.lo[a] = e.lo[a];
    }
    return FN;
}

// Inside the block the fine cells are a uniform grid of 2 q cells a side whose sub-layers carry the patterns of setRaysRefined
// (transportRoutinesModule.f90:150-187): the brick kernel sweeps it like a grid of its own (plan_brick_groups with a SubGridPlan),
// rays cross its faces through rings of its own face block, and the forest keeps what lies around it.  Fills H.fine (plan, stage
// lists per pipeline, the map from fine cells to leaves) and tells the boxes about the block.
int plan_fine_block(const HybridInputs &in, const Extent &cluster, int fine_chunk, const std::vector<int> &half_of_group, HybridPlan &H,
                    Boxes &boxes, std::string *err)
{
    HybridPlan::Fine &FN = H.fine;
    const BrickPlan &P = H.bricks;
    const int n = in.n, nf = FN.n;
    SubGridPlan sg;
    sg.n = nf;
    sg.cell = in.box / (double)n / 2.0; // the size of a cell halves per level (transportRoutinesModule.f90:583)
    sg.patterns = [n, nf, cluster](int, double phi_f, double theta_f, int izone, ftte_pattern *out) -> int {
        // the base layers the block spans along this izone's march axis, each with its two sub-layers
        ZoneMap zm;
        zone_map(izone, &zm);
        int lo0 = 1;
        for (int a = 0; a < 3; ++a)
            if (zm.src[a] == 0) lo0 = zm.mirror[a] ? n + 1 - cluster.hi[a] : cluster.lo[a];
        std::vector<ftte_pattern> base((size_t)n);
        if (layer_patterns(n, phi_f, theta_f, base.data())) return FTTE_ERR_PATTERN;
        for (int i = 0; i < nf / 2; ++i)
            if (sub_layer_patterns(base[(size_t)(lo0 - 1 + i)], phi_f, theta_f, &out[2 * i], &out[2 * i + 1])) return FTTE_ERR_PATTERN;
        return 0;
    };
    H.brick_plans_made = 2;
    // share 0, an accumulator per group: the fine grid is small and every launch a plain store
    const int rc = plan_brick_groups(FN.plan, n, in.box, in.ndir, in.phi, in.theta, in.w, fine_chunk, in.gmax, 0, 0, true, &sg, err);
    if (rc) return rc;
    BrickPlan &Q = FN.plan;
    if (Q.groups.size() != P.groups.size()) return fail(err, FTTE_ERR_STATE, "hybrid plan: the fine block's groups differ from the base grid's");
    Q.face_elems = Q.uqface_off; // (no boxes inside the fine grid)
    FN.face_base = P.face_elems;
    // stage lists per pipeline: list l = pipeline * nstages + stage, stage = tu + tv + ti, the groups with the most directions first
    // (an accumulator per group: nobody accumulates)
    FN.nstages = Q.ntu + Q.ntv + Q.nti - 2;
    const size_t nst = (size_t)FN.nstages;
    FN.stage_off = build_task_lists(Q, largest_groups_first(Q), (size_t)H.nhalves * nst, [&](size_t g, auto put) {
        for_each_brick(Q, [&](int tu, int tv, int ti) {
            const size_t st = (size_t)(tu + tv + ti);
            put((size_t)half_of_group[g] * nst + st, st, tu, tv, ti, BrickTask{(int16_t)g, (int16_t)tu, (int16_t)tv, (int16_t)ti});
        });
    });
    FN.updates = (int64_t)nf * nf * nf * in.ndir;
    // the boxes learn about the block: its extent in their sweep frame (the refined cells' own) and the fine face block
    for (auto &BX : boxes)
        for (HybridBox &B : BX) {
            ForestRegion &R = B.R;
            R.has_fine = true;
            for (int a = 0; a < 3; ++a) { R.flo[a] = B.fine.lo[a]; R.fhi[a] = B.fine.hi[a]; }
            R.fine.chunk = Q.chunk; R.fine.ut = Q.ut; R.fine.nslot = Q.nslot; R.fine.ntu = Q.ntu; R.fine.ntv = Q.ntv; R.fine.up = Q.up; R.fine.vp = Q.vp;
            R.fine.vface_off = Q.vface_off; R.fine.iface_off = Q.iface_off; R.fine.base = FN.face_base;
        }
    // fine cell (storage order inside the block) -> leaf: the children of a refined base cell follow each other in the cell array
    // in storage order 4 (a - 1) + 2 (b - 1) + (c - 1) (equiSources.f90:4044-4079)
    const AmrTree &tree = *in.tree;
    FN.leaf_of_fine.resize((size_t)nf * nf * nf);
    for (int a = 0; a < nf; ++a)
        for (int b = 0; b < nf; ++b)
            for (int d = 0; d < nf; ++d) {
                const int32_t node = (int32_t)(((int64_t)(FN.lo[0] - 1 + a / 2) * n + (FN.lo[1] - 1 + b / 2)) * n + (FN.lo[2] - 1 + d / 2));
                FN.leaf_of_fine[((size_t)a * nf + b) * nf + d] = tree.leaf[(size_t)(tree.child0[(size_t)node] + 4 * (a % 2) + 2 * (b % 2) + (d % 2))];
            }
    return FTTE_OK;
}

// What a group sweeps of brick (tu, tv, ti): nothing (a box holds it), all of it, or -- a box cuts through it along u -- the
// lanes on the near side of that box and / or those on the far side.  Every piece runs in the phase after the last pass it
// depends on: 1 + the highest level among the boxes it lies behind (phase 0: behind none).
struct Piece { int lane_lo, lane_hi, phase, box; bool masked; };
int pieces_of(int n, const std::vector<HybridBox> &BX, int tu, int tv, int ti, Piece out[2])
{
    const int last = std::min(63, n - 64 * tu - 1); // last lane with a cell
    int behind_all = 0, cut = -1;
    for (size_t x = 0; x < BX.size(); ++x) {
        const HybridBox &B = BX[x];
        if (tu >= B.lo[0] && tv >= B.lo[1] && ti >= B.lo[2]) behind_all = std::max(behind_all, B.level + 1);
        if (tv >= B.lo[1] && tv <= B.hi[1] && ti >= B.lo[2] && ti <= B.hi[2] && B.ulo <= 64 * tu + 64 && B.uhi >= 64 * tu + 1) cut = (int)x;
    }
    if (cut < 0) { out[0] = Piece{0, 63, behind_all, 0, false}; return 1; } // no box reaches into this brick
    const HybridBox &X = BX[(size_t)cut];
    const int first_in = std::max(X.ulo, 64 * tu + 1) - (64 * tu + 1), last_in = std::min(X.uhi, 64 * tu + 64) - (64 * tu + 1);
    int count = 0;
    if (first_in > 0) { // the near side: not behind the box it belongs to
        int behind_others = 0;
        for (size_t x = 0; x < BX.size(); ++x)
            if ((int)x != cut && tu >= BX[x].lo[0] && tv >= BX[x].lo[1] && ti >= BX[x].lo[2]) behind_others = std::max(behind_others, BX[x].level + 1);
        out[count++] = Piece{0, first_in - 1, behind_others, cut, true};
    }
    if (last_in < last) out[count++] = Piece{last_in + 1, 63, behind_all, cut, true};
    return count;
}
// every piece of every brick, in the order the task lists are written in: fn(tu, tv, ti, q, piece)
template <typename F> void for_each_piece(int n, const BrickPlan &P, const std::vector<HybridBox> &BX, F fn)
{
    for (int ti = 0; ti < P.nti; ++ti)
        for (int tv = 0; tv < P.ntv; ++tv)
            for (int tu = 0; tu < P.ntu; ++tu) {
                Piece pc[2];
                const int np = pieces_of(n, BX, tu, tv, ti, pc);
                for (int q = 0; q < np; ++q) fn(tu, tv, ti, q, pc[q]);
            }
}

// the box that holds lanes [lane_lo, lane_hi] of brick (tu, tv, ti), or -1
int box_over(const std::vector<HybridBox> &BX, int tu, int tv, int ti, int lane_lo, int lane_hi)
{
    for (size_t x = 0; x < BX.size(); ++x) {
        const HybridBox &B = BX[x];
        if (tv >= B.lo[1] && tv <= B.hi[1] && ti >= B.lo[2] && ti <= B.hi[2] && B.ulo <= 64 * tu + 1 + lane_hi && B.uhi >= 64 * tu + 1 + lane_lo) return (int)x;
    }
    return -1;
}

// ---- slots (several passes).  A piece's slot is the first launch after everything it takes rays from: the pieces of the three
// bricks upstream that share lanes with it, and the forests of the boxes directly upstream of it (pass k of a pipeline is
// issued in front of the launches of slot pass_at[k], which lies behind every piece that feeds a box of level k in that
// pipeline).  Level after level, because a pass's place needs the slots of its feeders and its consumers' slots need its place.
// Fills slot[group][2 brick + piece] and H.pass_at; *nslots: how many launch lists that makes.
int assign_slots(int n, const BrickPlan &P, const Boxes &boxes, const std::vector<int> &half_of_group, HybridPlan &H,
                 std::vector<std::vector<int32_t>> &slot, int *nslots, std::string *err)
{
    const size_t nb = (size_t)P.ntu * P.ntv * P.nti;
    for (size_t g = 0; g < P.groups.size(); ++g) slot[g].assign(2 * nb, -1);
    for (int k = 0; k <= H.npass; ++k) {
        for (size_t g = 0; g < P.groups.size(); ++g) {
            const std::vector<HybridBox> &BX = boxes[g];
            const std::vector<int> &at = H.pass_at[(size_t)half_of_group[g]];
            std::vector<int32_t> &S = slot[g];
            for_each_piece(n, P, BX, [&](int tu, int tv, int ti, int q, const Piece &pc) {
                int32_t &mine = S[2 * brick_index(P, tu, tv, ti) + (size_t)q];
                if (mine >= 0) return;
                int s2 = 0;
                bool known = true;
                auto after_pass = [&](int x) { if (BX[(size_t)x].level >= k) known = false; else s2 = std::max(s2, at[(size_t)BX[(size_t)x].level]); };
                // the brick on the near side along u, or (lanes that start inside the brick) the box there
                if (pc.lane_lo > 0) after_pass(pc.box);
                else if (tu > 0) {
                    Piece up[2];
                    const int nu2 = pieces_of(n, BX, tu - 1, tv, ti, up);
                    if (nu2 > 0 && up[nu2 - 1].lane_hi == 63) {
                        const int32_t v = S[2 * brick_index(P, tu - 1, tv, ti) + (size_t)(nu2 - 1)];
                        if (v < 0) known = false; else s2 = std::max(s2, v + 1);
                    } else { const int x = box_over(BX, tu - 1, tv, ti, 63, 63); if (x >= 0) after_pass(x); }
                }
                // the bricks below along v and the march axis: their pieces that share lanes, and the box between them
                for (int axis = 1; axis <= 2; ++axis) {
                    const int nv = axis == 1 ? tv - 1 : tv, ni = axis == 2 ? ti - 1 : ti;
                    if (nv < 0 || ni < 0) continue;
                    Piece up[2];
                    const int nu2 = pieces_of(n, BX, tu, nv, ni, up);
                    for (int r = 0; r < nu2; ++r)
                        if (up[r].lane_lo <= pc.lane_hi && up[r].lane_hi >= pc.lane_lo) {
                            const int32_t v = S[2 * brick_index(P, tu, nv, ni) + (size_t)r];
                            if (v < 0) known = false; else s2 = std::max(s2, v + 1);
                        }
                    const int x = box_over(BX, tu, nv, ni, pc.lane_lo, pc.lane_hi);
                    if (x >= 0) after_pass(x);
                }
                if (known) mine = s2;
            });
        }
        if (k == H.npass) break;
        // where pass k goes: behind every piece that hands rays to a box of level k
        for (size_t g = 0; g < P.groups.size(); ++g) {
            const std::vector<HybridBox> &BX = boxes[g];
            int &at = H.pass_at[(size_t)half_of_group[g]][(size_t)k];
            if (k > 0) at = std::max(at, H.pass_at[(size_t)half_of_group[g]][(size_t)k - 1]);
            bool late = false;
            for_each_piece(n, P, BX, [&](int tu, int tv, int ti, int q, const Piece &pc) {
                bool feeds = false;
                if (pc.lane_hi < 63) feeds = BX[(size_t)pc.box].level == k; // lanes that end inside the brick: at a box
                else if (tu + 1 < P.ntu) { const int x = box_over(BX, tu + 1, tv, ti, 0, 0); feeds = x >= 0 && BX[(size_t)x].level == k; }
                if (!feeds && tv + 1 < P.ntv) { const int x = box_over(BX, tu, tv + 1, ti, pc.lane_lo, pc.lane_hi); feeds = x >= 0 && BX[(size_t)x].level == k; }
                if (!feeds && ti + 1 < P.nti) { const int x = box_over(BX, tu, tv, ti + 1, pc.lane_lo, pc.lane_hi); feeds = x >= 0 && BX[(size_t)x].level == k; }
                if (!feeds) return;
                const int32_t v = slot[g][2 * brick_index(P, tu, tv, ti) + (size_t)q];
                if (v < 0) late = true;
                at = std::max(at, v + 1);
            });
            if (late) return fail(err, FTTE_ERR_STATE, "hybrid plan: a brick that feeds a box waits for a later pass");
        }
    }
    *nslots = 0;
    for (size_t g = 0; g < P.groups.size(); ++g)
        for (int32_t v : slot[g]) *nslots = std::max(*nslots, v + 1);
    for (auto &at : H.pass_at) for (int v : at) *nslots = std::max(*nslots, v);
    return FTTE_OK;
}

// The tasks: the bricks outside the boxes, and what the boxes leave of the bricks they cut through.  A pipeline's launch lists go by
// slot, or (one pass, or slots switched off) by phase -- phase 0: what lies behind no box, phase k: what needs the forests up to
// pass k - 1 -- and within a phase stage by stage as in a plain sweep.
// Two sets of lists in one task array, [whole lists][masked lists]: the masked kernel (a lane range per task)
// takes every brick of a stage in which some brick is cut by a box -- two launches per stage would run one after the other,
// and a launch of a few bricks lasts as long as one of many --, the plain kernel the stages without.
// Fills P.tasks, H.stage_off and H.brick_updates (H.nlist, nhalves and pass_at are settled).
void write_task_lists(int n, BrickPlan &P, const Boxes &boxes, const std::vector<int> &half_of_group, const std::vector<std::vector<int32_t>> &slot,
                      int per_phase, HybridPlan &H)
{
    const size_t nlist = (size_t)H.nhalves * H.nlist;
    auto list_of = [&](size_t g, const Piece &pc, int tu, int tv, int ti, int q) {
        if (H.slots) return (size_t)half_of_group[g] * H.nlist + (size_t)slot[g][2 * brick_index(P, tu, tv, ti) + (size_t)q];
        return (size_t)half_of_group[g] * H.nlist + (size_t)pc.phase * (size_t)per_phase + (size_t)(tu + tv + ti + P.groups[g].offset);
    };
    // the lists in which some brick is cut by a box go to the masked half, all of their tasks with a lane range
    std::vector<uint8_t> cut(nlist, 0);
    H.brick_updates = 0;
    for (size_t g = 0; g < P.groups.size(); ++g)
        for_each_piece(n, P, boxes[g], [&](int tu, int tv, int ti, int q, const Piece &pc) {
            if (pc.masked) cut[list_of(g, pc, tu, tv, ti, q)] = 1;
            const int64_t cu = std::max(0, std::min(pc.lane_hi, n - 64 * tu - 1) - pc.lane_lo + 1), cv = std::min(kBrickRows, n - kBrickRows * tv),
                          ci = std::min(P.chunk, n - P.chunk * ti);
            H.brick_updates += cu * cv * ci * (int64_t)P.groups[g].dirs.size();
        });
    H.stage_off = build_task_lists(P, groups_in_order(P), 2 * nlist, [&](size_t g, auto put) {
        for_each_piece(n, P, boxes[g], [&](int tu, int tv, int ti, int q, const Piece &pc) {
            const size_t l = list_of(g, pc, tu, tv, ti, q);
            BrickTask T;
            T.tv = (int16_t)(cut[l] ? tv | (pc.box << kBrickBoxShift) : tv);
            T.group = (int16_t)(cut[l] ? (int)g | (pc.lane_hi << kBrickLaneHiShift) : (int)g);
            T.tu = (int16_t)(uint16_t)(cut[l] ? tu | (pc.lane_lo << kBrickLaneLoShift) : tu);
            T.ti = (int16_t)ti;
            put((cut[l] ? nlist : 0) + l, l, tu, tv, ti, T);
        });
    });
}

// The forests, restricted to the boxes: linked on the host a few directions at a time.  Once the leaves that lie in any box are
// known they are numbered by their place in that list, and segments (3 * place + piece), activity bytes, opacities and scratch
// use those numbers: what the forests need of memory follows the boxes, not the tree.  Fills H.dirs and H.cells from H.regions.
int link_forests(const HybridInputs &in, HybridPlan &H, std::string *err)
{
    const BrickPlan &P = H.bricks;
    const AmrTree &tree = *in.tree;
    const int ndir = in.ndir;
    const int64_t ncell = tree.ncell;
    std::vector<int> group_of((size_t)ndir, -1);
    for (size_t g = 0; g < P.groups.size(); ++g) for (int d : P.groups[g].dirs) group_of[(size_t)d] = (int)g;
    H.dirs.assign((size_t)ndir, HybridPlan::Dir());
    H.forests_linked = true;
    const int nthreads = std::max(1u, std::min(16u, std::thread::hardware_concurrency()));
    std::vector<uint8_t> in_any((size_t)ncell, 0);
    // per direction: which pieces the leaves it walked have, and whether they are the forest's (every other leaf: not the forest's)
    std::vector<std::vector<std::pair<int32_t, uint8_t>>> active((size_t)ndir);
    static_assert(sizeof(AmrForest::Export) == sizeof(AmrExport), "export records: host and device forms must agree");
    static_assert(sizeof(AmrForest::FineImport) == sizeof(AmrImport), "import records: host and device forms must agree");
    {
        // a thread keeps its forest from direction to direction: after the first, a build touches only what the boxes hold (ftte_amr.h)
        const int nt = std::min(nthreads, ndir);
        std::vector<int> st((size_t)ndir, 0);
        std::vector<std::string> msg((size_t)ndir);
        std::vector<std::vector<int32_t>> seen((size_t)nt); // leaves inside a box of at least one of the thread's directions
        std::vector<std::thread> pool;
        for (int t = 0; t < nt; ++t)
            pool.emplace_back([&, t] {
                AmrForest f;
                for (int d = t; d < ndir; d += nt) {
                    const DirPlan &D = P.dirs[(size_t)d];
                    st[(size_t)d] = build_forest_regions(tree, D.phi, D.theta, D.izone, in.box, &f, &msg[(size_t)d], H.regions[(size_t)group_of[(size_t)d]]);
                    if (st[(size_t)d]) return;
                    HybridPlan::Dir &HD = H.dirs[(size_t)d];
                    HD.rec = pack_segments(f);
                    active[(size_t)d].reserve(f.visited.size());
                    for (int32_t q : f.visited) {
                        active[(size_t)d].push_back({q, (uint8_t)((f.up[3 * (size_t)q + 1] != AmrForest::kInactive ? 1 : 0) | (f.up[3 * (size_t)q + 2] != AmrForest::kInactive ? 2 : 0) |
                                                                  (f.inside[(size_t)q] ? 0 : 4))});
                        if (f.inside[(size_t)q]) seen[(size_t)t].push_back(q);
                    }
                    HD.depth_off = f.depth_off;
                    HD.pass_first = f.pass_first;
                    HD.export_first = f.export_first;
                    HD.exports.resize(f.exports.size());
                    if (!f.exports.empty()) std::memcpy(HD.exports.data(), f.exports.data(), sizeof(AmrExport) * f.exports.size());
                    HD.imports.resize(f.fine_imports.size());
                    if (!f.fine_imports.empty()) std::memcpy(HD.imports.data(), f.fine_imports.data(), sizeof(AmrImport) * f.fine_imports.size());
                }
            });
        for (auto &th : pool) th.join();
        for (int d = 0; d < ndir; ++d)
            if (st[(size_t)d]) return fail(err, st[(size_t)d], "direction " + std::to_string(d) + ": " + msg[(size_t)d]);
        for (const auto &list : seen) for (int32_t q : list) in_any[(size_t)q] = 1;
    }
    std::vector<int32_t> &cells = H.cells;
    std::vector<int32_t> place((size_t)ncell, -1);
    cells.clear();
    for (int64_t q = 0; q < ncell; ++q)
        if (in_any[(size_t)q]) { place[(size_t)q] = (int32_t)cells.size(); cells.push_back((int32_t)q); }
    auto renumber = [&](int32_t sg) { return sg < 0 ? sg : 3 * place[(size_t)(sg / 3)] + sg % 3; }; // negative: inflow / import marks
    std::vector<int> bad((size_t)ndir, 0);
    std::vector<std::thread> pool;
    for (int t = 0; t < nthreads; ++t)
        pool.emplace_back([&, t] {
            for (int d = t; d < ndir; d += nthreads) {
                HybridPlan::Dir &HD = H.dirs[(size_t)d];
                for (SegRec &R : HD.rec) {
                    if (place[(size_t)(R.seg / 3)] < 0 || (R.up >= 0 && place[(size_t)(R.up / 3)] < 0) || (R.up2 >= 0 && place[(size_t)(R.up2 / 3)] < 0)) { bad[(size_t)d] = 1; break; }
                    R.seg = renumber(R.seg); R.up = renumber(R.up); R.up2 = renumber(R.up2);
                }
                for (AmrExport &X : HD.exports) {
                    if (place[(size_t)(X.seg / 3)] < 0) { bad[(size_t)d] = 1; break; }
                    X.seg = renumber(X.seg);
                }
                for (AmrImport &X : HD.imports) {
                    if ((X.up >= 0 && place[(size_t)(X.up / 3)] < 0) || (X.up2 >= 0 && place[(size_t)(X.up2 / 3)] < 0)) { bad[(size_t)d] = 1; break; }
                    X.up = renumber(X.up); X.up2 = renumber(X.up2);
                }
                // the activity bytes of the leaves in `cells`
                HD.active.assign(cells.size(), (uint8_t)4);
                for (const auto &a : active[(size_t)d]) if (place[(size_t)a.first] >= 0) HD.active[(size_t)place[(size_t)a.first]] = a.second;
            }
        });
    for (auto &th : pool) th.join();
    for (int d = 0; d < ndir; ++d)
        if (bad[(size_t)d]) return fail(err, FTTE_ERR_STATE, "hybrid plan: a forest segment lies outside every box");
    return FTTE_OK;
}

} // namespace

int plan_hybrid(const HybridInputs &in, HybridPlan &H, std::string *err)
{
    const int n = in.n, ndir = in.ndir;
    BrickPlan &P = H.bricks;
    int rc;
    H.brick_plans_made = 1;
    if ((rc = plan_brick_groups(P, n, in.box, ndir, in.phi, in.theta, in.w, in.chunk, in.gmax, in.share, 0, true, nullptr, err))) return rc;
    P.glanes = 1;
    const std::vector<Extent> clusters = refined_clusters(*in.tree);
    Boxes boxes = boxes_of_groups(n, in.opt.lanes, P, clusters, H);
    H.valid = true;
    if (!H.worthwhile) return FTTE_OK;
    H.slots = slot_form(in.opt, ndir, H.npass, P);
    const std::vector<int> half_of_group = deal_pipelines(P, in.opt.pipelines, ndir, &H.half_dirs);
    H.nhalves = (int)H.half_dirs.size();
    const int fine_chunk = in.opt.fine_chunk > 0 ? in.opt.fine_chunk : in.chunk; // layers per brick on the fine level (option "fine_chunk")
    H.fine = fine_block_of(*in.tree, clusters, in.opt.fine_bricks && H.npass == 1 && !H.slots, fine_chunk);
    if (H.fine.active && (rc = plan_fine_block(in, clusters[0], fine_chunk, half_of_group, H, boxes, err))) return rc;

    int max_offset = 0;
    for (const auto &G : P.groups) max_offset = std::max(max_offset, G.offset);
    const int per_phase = P.ntu + P.ntv + P.nti - 2 + max_offset;
    H.phase1_stages = (size_t)per_phase;
    std::vector<std::vector<int32_t>> slot(P.groups.size());
    H.pass_at.assign((size_t)H.nhalves, std::vector<int>((size_t)H.npass, 0));
    int nslots = 0;
    if (H.slots && (rc = assign_slots(n, P, boxes, half_of_group, H, slot, &nslots, err))) return rc;
    // the launch lists of a pipeline: a piece's slot, or (one pass, or slots switched off) a phase per pass, in it the stages of a
    // plain sweep: phase 0 before the first pass of the forests, phase k after pass k - 1
    H.nlist = H.slots ? (size_t)std::max(nslots, 1) : (size_t)(H.npass + 1) * (size_t)per_phase;
    if (!H.slots) for (auto &at : H.pass_at) for (int k = 0; k < H.npass; ++k) at[(size_t)k] = (k + 1) * per_phase;
    write_task_lists(n, P, boxes, half_of_group, slot, per_phase, H);
    if (P.ntu > kBrickTuMask || P.ntv > kBrickTvMask || (int)P.groups.size() > kBrickGroupMask)
        return fail(err, FTTE_ERR_UNSUPPORTED, "hybrid sweep: more than 1023 bricks along a row, or more than 255 groups of directions");
    H.regions.assign(boxes.size(), std::vector<ForestRegion>());
    for (size_t g = 0; g < boxes.size(); ++g) for (const HybridBox &B : boxes[g]) H.regions[g].push_back(B.R);
    return link_forests(in, H, err);
}

} // namespace ftte
