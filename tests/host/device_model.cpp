// device_model.cpp -- host definitions of the launches (ftte_*_rec.h, ftte_layout.h) that the sweeps of a refined cell array reach
// (ftte_sweeps.cpp: forest_sweep; ftte_hybrid.cpp: hybrid_sweep), for programs that link those sources against the stub of the HIP
// runtime (tests/host/stub): "device" memory is malloc there, so under the address sanitizer every index the host code hands to
// the device becomes a checked access.
//
// The launches for the forests and the medium copies are serial loops over the (thread -> element) mapping of their kernels
// (ftte_forest.hip, ftte_layout.hip), with the arithmetic of ftte_math.h: they dereference the addresses the kernels dereference.
//
// launch_brick is NOT a transcription of the brick kernel.  It is an oracle brick: the program that drives the model has evaluated
// the whole tree direction by direction (model::DirOracle), and for every task, direction and frequency group of a launch the
// oracle brick
//  * reads every face element the kernel takes rays from (u_in, v_in, i_in at the offsets of BrickLaunch, ftte_brick_rec.h) and
//    requires it to hold, bit for bit, the oracle's incoming intensity of the cell that receives it;
//  * writes the oracle's value into every face element the kernel hands rays on through (u_out, v_out, i_out);
//  * adds the oracle's cell means into the accumulator at the address the kernel forms from the group record.
// The ray that enters base cell X through face f (0: from layer i - 1, 1: from j - 1, 2: from k - 1, sweep frame) is the incoming
// intensity of X's segment f.  Which cell a (brick, layer, row, lane) is follows from the izone's frame (zone_map) and is compared
// with what the group record's org and strides say: a second statement of the contract, not the planner's.
//
// The launches no refined-grid path reaches print a message and abort.  tests/host/ only.
#include "device_model.h"

#include <cstdarg>
#include <cstdio>
#include <cstdlib>

namespace model {

State &state() { static State s; return s; }

static void found(const char *fmt, ...) __attribute__((format(printf, 1, 2)));
static void found(const char *fmt, ...)
{
    State &S = state();
    ++S.failures;
    if (!S.first.empty()) return;
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    std::vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    S.first = buf;
}
[[noreturn]] static void unreachable_launch(const char *what)
{
    std::fprintf(stderr, "ERROR device model: %s was launched: no sweep of a refined cell array reaches it\n", what);
    std::abort();
}
// a load the compiler keeps: the kernel loads the element whatever it does with it
static inline double touch(const double *p) { return *(const volatile double *)p; }

} // namespace model

namespace ftte {

using model::found;
using model::state;
using model::touch;

bool brick_whole_form(const BrickLaunch &, int, bool) { return false; }
int launch_sweep(const LaunchRec &, int, int, int, int, int, hipStream_t) { model::unreachable_launch("launch_sweep"); }
int launch_brick_pair(const BrickLaunch &, int, int, int, hipStream_t) { model::unreachable_launch("launch_brick_pair"); }
int launch_merge_blocks(const double *const *, const int *, int, double *, int, int, long, const int32_t *, int, int, hipStream_t, bool, int)
{
    model::unreachable_launch("launch_merge_blocks");
}
int launch_xcc_census(unsigned *, hipStream_t) { model::unreachable_launch("launch_xcc_census"); }

// ---- the medium copies -------------------------------------------------------------------------------------------------
int launch_cell_major(const double *src, double *dst, long ncell, int nnu, hipStream_t, const int32_t *cells, long count)
{
    if (!cells) count = ncell;
    if (count <= 0) return 0;
    for (long c = 0; c < count; ++c)
        for (int g = 0; g < nnu; ++g) dst[c * nnu + g] = src[(long)g * ncell + (cells ? (long)cells[c] : c)];
    return 0;
}

int launch_base_cells(const double *leaf_values, const int32_t *leaf_of_base, double *base_values, long nbase, long ncell, int nnu, hipStream_t)
{
    for (long g = 0; g < nnu; ++g)
        for (long b = 0; b < nbase; ++b) {
            const int32_t leaf = leaf_of_base[b];
            base_values[g * nbase + b] = leaf >= 0 ? leaf_values[g * ncell + leaf] : 0.0;
        }
    return 0;
}

int launch_to_layout(int layout, const double *src, double *dst, int n, int nnu, long group_stride, hipStream_t, bool tiled, int)
{
    if (tiled) { std::fprintf(stderr, "ERROR device model: launch_to_layout in brick order: nothing on a refined cell array sets it\n"); std::abort(); }
    if (layout != 1 && layout != 2) return -1;
    for (long g = 0; g < nnu; ++g)
        for (long ic = 0; ic < n; ++ic)
            for (long jc = 0; jc < n; ++jc)
                for (long kc = 0; kc < n; ++kc) {
                    const double v = src[g * group_stride + (ic * n + jc) * n + kc];
                    if (layout == 1) dst[g * group_stride + (jc * n + ic) * n + kc] = v;
                    else dst[g * group_stride + (kc * n + ic) * n + jc] = v;
                }
    return 0;
}

int launch_merge(const double *const *acc, const int *layout, int count, double *J, int n, int nnu, long group_stride, bool accumulate, hipStream_t,
                 const int32_t *leaf_of_base, long j_stride, bool tiled, int)
{
    if (count > 3 * kMaxAcc) return -1;
    if (tiled) { std::fprintf(stderr, "ERROR device model: launch_merge in brick order: nothing on a refined cell array sets it\n"); std::abort(); }
    for (long g = 0; g < nnu; ++g)
        for (long ic = 0; ic < n; ++ic)
            for (long jc = 0; jc < n; ++jc)
                for (long kc = 0; kc < n; ++kc) {
                    const long b = (ic * n + jc) * n + kc;
                    double sum = 0.0;
                    bool have = false;
                    if (accumulate && !leaf_of_base) { sum = J[g * group_stride + b]; have = true; }
                    for (int a = 0; a < count; ++a) {
                        const double *s = acc[a] + g * group_stride;
                        const double v = layout[a] == 0 ? s[b] : layout[a] == 1 ? s[(jc * n + ic) * n + kc] : s[(kc * n + ic) * n + jc];
                        sum = have ? sum + v : v;
                        have = true;
                    }
                    if (!leaf_of_base) J[g * group_stride + b] = sum;
                    else if (leaf_of_base[b] >= 0) {
                        double *dst = &J[g * j_stride + leaf_of_base[b]];
                        *dst = accumulate ? *dst + sum : sum;
                    }
                }
    return 0;
}

// ---- the forests ---------------------------------------------------------------------------------------------------------
// amr_segment: segment e of the level that starts at `begin` in direction D's list, frequency group nu
static void amr_segment(const AmrLevelRec &A, const AmrDirRec &D, int64_t begin, unsigned e, unsigned nu, unsigned nnu)
{
    const SegRec R = D.rec[begin + e];
    const int seg = R.seg, up = R.up, up2 = R.up2;
    const size_t at = (size_t)(unsigned)seg * nnu + nu;
    double I;
    if (up == -3) I = D.faces[(size_t)nu * A.face_stride + (size_t)R.at];
    else if (up < 0) I = A.uvb[nu];
    else {
        I = D.Iout[(size_t)(unsigned)up * nnu + nu];
        if (up2 >= 0) I = 0.5 * (I + D.Iout[(size_t)(unsigned)up2 * nnu + nu]);
    }
    const unsigned cell = (unsigned)seg / 3u;
    const size_t kat = (size_t)nu * A.group_stride + (size_t)cell * A.cell_stride;
    const double kap = A.kappa[kat];
    double m;
    if (A.emit == 0) m = ftte_segment(&A.math, &I, kap * R.dpath);
    else {
        const double x = A.emis[kat];
        m = A.emit == 2 ? ftte_segment_source(&A.math, A.math.c[9], &I, kap * R.dpath, x) : ftte_segment_emit(&A.math, &I, kap * R.dpath, x, 0.0);
    }
    D.Iout[at] = I;
    D.mean[at] = m;
}

int launch_amr_level(const AmrLevelRec &A, hipStream_t)
{
    if (A.most <= 0) return 0;
    const int64_t threads = A.most * A.nnu;
    if (threads >= ((int64_t)1 << 32)) return -1;
    const uint64_t launched = (uint64_t)((threads + 255) / 256) * 256; // threads per direction: a level fuller than `most` says is cut short
    const unsigned nnu = (unsigned)A.nnu;
    ++state().levels;
    for (int d = 0; d < A.ndir; ++d) {
        const unsigned count = (unsigned)A.count[d];
        const int64_t begin = A.begin[d];
        for (uint64_t t = 0; t < launched && t / nnu < count; ++t) amr_segment(A, A.dir[d], begin, (unsigned)(t / nnu), (unsigned)(t % nnu), nnu);
    }
    return 0;
}

int launch_amr_levels(const AmrLevelRec &A, const int64_t *tables, int ndepth, hipStream_t)
{
    if (ndepth <= 0 || A.ndir <= 0) return 0;
    const unsigned nnu = (unsigned)A.nnu;
    ++state().fused;
    for (int d = 0; d < A.ndir; ++d) {
        const AmrDirRec &D = A.dir[d];
        for (int k = 0; k < ndepth; ++k) {
            const int64_t *T = tables + (size_t)k * 2 * (size_t)A.ndir;
            const unsigned items = (unsigned)T[d] * nnu;
            const int64_t begin = T[A.ndir + d];
            for (unsigned t = 0; t < items; ++t) amr_segment(A, D, begin, t / nnu, t % nnu, nnu);
        }
    }
    return 0;
}

int launch_amr_combine(const AmrLevelRec &A, double *J, bool zero_first, hipStream_t)
{
    const long slots = A.cells ? A.ncells : A.ncell;
    const int nnu = A.nnu;
    for (long slot = 0; slot < slots; ++slot)
        for (int nu = 0; nu < nnu; ++nu) {
            const long cell = A.cells ? A.cells[slot] : slot;
            double acc_J = zero_first ? 0.0 : J[(long)nu * A.ncell + cell];
            for (int d = 0; d < A.ndir; ++d) {
                const AmrDirRec &D = A.dir[d];
                const int active = D.active[slot];
                if (active & 4) continue;
                double acc = D.mean[(3 * slot) * nnu + nu];
                int nseg = 1;
                if (active & 1) { acc += D.mean[(3 * slot + 1) * nnu + nu]; ++nseg; }
                if (active & 2) { acc += D.mean[(3 * slot + 2) * nnu + nu]; ++nseg; }
                acc_J += ftte_cell_mean(acc, nseg, D.w);
            }
            J[(long)nu * A.ncell + cell] = acc_J;
        }
    return 0;
}

int launch_amr_export(const AmrLevelRec &A, int64_t most, hipStream_t)
{
    if (most <= 0) return 0;
    const long launched = (long)((most * A.nnu + 255) / 256) * 256;
    const int nnu = A.nnu;
    ++state().exports;
    for (int d = 0; d < A.ndir; ++d) {
        const AmrDirRec &D = A.dir[d];
        const long count = A.count ? (long)A.count[d] : (long)D.nexports, first = A.begin ? (long)A.begin[d] : 0l;
        for (long t = 0; t < launched && t / nnu < count; ++t) {
            const long e = t / nnu;
            const int nu = (int)(t - e * nnu);
            const AmrExport X = D.exports[first + e];
            D.faces[(size_t)nu * A.face_stride + (size_t)X.at] = D.Iout[(size_t)(unsigned)X.seg * nnu + nu];
        }
    }
    return 0;
}

int launch_amr_fine_import(const AmrLevelRec &A, int64_t most, hipStream_t)
{
    if (most <= 0) return 0;
    const long launched = (long)((most * A.nnu + 255) / 256) * 256;
    const int nnu = A.nnu;
    ++state().imports;
    for (int d = 0; d < A.ndir; ++d) {
        const AmrDirRec &D = A.dir[d];
        for (long t = 0; t < launched && t / nnu < (long)D.nimports; ++t) {
            const long e = t / nnu;
            const int nu = (int)(t - e * nnu);
            const AmrImport X = D.imports[e];
            double I;
            if (X.up < 0) I = A.uvb[nu];
            else {
                I = D.Iout[(size_t)(unsigned)X.up * nnu + nu];
                if (X.up2 >= 0) I = 0.5 * (I + D.Iout[(size_t)(unsigned)X.up2 * nnu + nu]);
            }
            D.faces[(size_t)nu * A.face_stride + (size_t)X.at] = I;
        }
    }
    return 0;
}

// ---- the oracle brick ----------------------------------------------------------------------------------------------------
namespace {

// One launch's view of a group: which array of cells it sweeps (the base grid or the fine block, in which layout), its frame
struct Frame {
    bool fine = false;
    int layout = 0, side = 0;
    ZoneMap zm;
    bool u_is_k = true;
    int u_slot = 2, v_slot = 1; // the segment that takes the ray crossing a u-face / a v-face
    const ftte_ctx *c = nullptr;

    // storage coordinates (1-based) of sweep-frame brick cell (i, v, u)
    void storage(int i, int v, int u, int (&st)[3]) const
    {
        const int sw[3] = {i, u_is_k ? v : u, u_is_k ? u : v};
        for (int a = 0; a < 3; ++a) st[a] = zm.mirror[a] ? side + 1 - sw[zm.src[a]] : sw[zm.src[a]];
    }
    // where the cell lies in the group's array of cells
    int64_t element(const int (&st)[3]) const
    {
        const int64_t s = side, a = st[0] - 1, b = st[1] - 1, k = st[2] - 1;
        return layout == 0 ? (a * s + b) * s + k : layout == 1 ? (b * s + a) * s + k : (k * s + a) * s + b;
    }
    // the leaf, or -1 for a refined base cell
    int32_t leaf(const int (&st)[3]) const
    {
        const AmrTree &T = c->tree;
        if (!fine) return T.leaf[(size_t)(((int64_t)(st[0] - 1) * side + (st[1] - 1)) * side + (st[2] - 1))];
        const HybridPlan::Fine &F = c->hplan.fine;
        const int a = st[0] - 1, b = st[1] - 1, k = st[2] - 1;
        const int64_t base = ((int64_t)(F.lo[0] - 1 + a / 2) * T.n + (F.lo[1] - 1 + b / 2)) * T.n + (F.lo[2] - 1 + k / 2);
        if (T.child0[(size_t)base] < 0) return -1;
        return T.leaf[(size_t)(T.child0[(size_t)base] + 4 * (a % 2) + 2 * (b % 2) + (k % 2))];
    }
};

bool has_u(int rc) { return rc == RC_TWO_U || rc == RC_THREE_U || rc == RC_THREE_V || rc == RC_THREE_U_SWAP || rc == RC_THREE_V_SWAP; }
bool has_v(int rc) { return rc == RC_TWO_V || rc == RC_THREE_U || rc == RC_THREE_V || rc == RC_THREE_U_SWAP || rc == RC_THREE_V_SWAP; }

} // namespace

int launch_brick(const BrickLaunch &L, int max_dirs, int, int, hipStream_t, bool masked, int persistent)
{
    model::State &S = state();
    if (!S.c) { std::fprintf(stderr, "ERROR device model: launch_brick without an oracle\n"); std::abort(); }
    if (persistent || L.ticket || L.queue || L.tiled || L.ablate || L.atomic_acc || L.through) {
        std::fprintf(stderr, "ERROR device model: launch_brick in a form no sweep of a refined cell array takes\n");
        std::abort();
    }
    const ftte_ctx &c = *S.c;
    const HybridPlan &H = c.hplan;
    constexpr int R = kBrickRows;
    const bool sub = !masked && L.sub != 0;
    const BrickPlan &P = sub ? H.fine.plan : H.bricks;
    const int n = L.n, chunk = L.chunk, up = L.up, vp = L.vp, ns = L.nslot, uw = L.uw, ut = L.ut, nnu_ctx = c.nnu;
    const double junk = model::from_bits(model::kJunkBits);
    if (n != P.n || L.nu0 < 0 || L.nu0 + L.nnu > nnu_ctx) found("launch_brick: n %d of a plan of %d, groups %d + %d of %d", n, P.n, L.nu0, L.nnu, nnu_ctx);
    const int64_t dir_elems = (int64_t)nnu_ctx * L.face_stride; // a direction's face block, all groups
    auto differs = [&](const double *e, double want, const char *what, int d, int nu, int i, int v, int u) {
        ++S.compared;
        const double got = touch(e);
        if (model::bits_of(got) == model::bits_of(want)) return;
        found("%s brick: %s of direction %d, group %d, cell (i %d, v %d, u %d) is element %lld of its face block and holds %a%s, the oracle has %a",
              sub ? "fine" : masked ? "masked" : "whole", what, d, nu, i, v, u, (long long)(e - (c.d_faces.get() + (int64_t)d * dir_elems + (int64_t)nu * L.face_stride)), got,
              model::bits_of(got) == model::kPoisonBits ? " (poison: nothing has written it)" : model::bits_of(got) == model::kJunkBits ? " (a ray of no cell)" : "", want);
    };

    std::vector<int32_t> leaf_of;
    for (int t = 0; t < L.ntasks; ++t) {
        const BrickTask &T = L.tasks[t];
        if ((const void *)&T == S.drop_task) continue;
        ++S.brick_tasks; if (masked) ++S.masked_tasks; if (sub) ++S.sub_tasks;
        const int tu_field = T.tu, group_field = T.group, tv_field = T.tv;
        const int tu = masked ? tu_field & kBrickTuMask : tu_field, lane_lo = masked ? (tu_field >> kBrickLaneLoShift) & 63 : 0;
        const int lane_hi = masked ? (group_field >> kBrickLaneHiShift) & 63 : 63;
        const int tv = masked ? tv_field & kBrickTvMask : tv_field, box = masked ? (tv_field >> kBrickBoxShift) & kBrickBoxMask : 0;
        const int ti = T.ti & (kBrickAccumulate - 1);
        const bool accumulate = (T.ti & kBrickAccumulate) != 0;
        const int gi = masked ? group_field & kBrickGroupMask : group_field;
        if (gi < 0 || gi >= (int)P.groups.size() || tu < 0 || tv < 0 || 64 * tu >= n || R * tv >= n || ti * chunk >= n) {
            found("launch_brick: task %d names group %d, brick (%d, %d, %d) of a grid of %d", t, gi, tu, tv, ti, n);
            continue;
        }
        const BrickGroup &G = L.groups[gi];
        const int ndir = G.ndir;
        if (ndir < 1 || ndir > max_dirs || ndir > kBrickMaxDirs) { found("launch_brick: group %d has %d directions, the launch is sized for %d", gi, ndir, max_dirs); continue; }

        // ---- the array of cells the group sweeps, and its frame
        Frame Fr;
        Fr.c = &c; Fr.side = n; Fr.layout = -1;
        for (int l = 0; l < 3; ++l)
            for (int s = 0; s < kMaxAcc; ++s) {
                if (G.J && G.J == c.acc[l][s].get()) { Fr.layout = l; Fr.fine = false; }
                if (G.J && G.J == c.hdev.fine_acc[l][s].get()) { Fr.layout = l; Fr.fine = true; }
            }
        if (Fr.layout < 0 || Fr.fine != sub) { found("launch_brick: the accumulator of group %d is none of the %s plan's", gi, sub ? "fine" : "base"); continue; }
        if (G.kappa != (sub ? c.hdev.fine_kappa[Fr.layout] : c.hdev.base_kappa[Fr.layout])) found("launch_brick: group %d reads opacities that are not its layout's", gi);
        if (L.emit && G.emis != (sub ? c.hdev.fine_emis[Fr.layout] : c.hdev.base_emis[Fr.layout])) found("launch_brick: group %d reads an emissivity that is not its layout's", gi);
        // the group's directions: which of the call's they are, by where their face blocks lie
        int dirs[kBrickMaxDirs];
        bool ok = true;
        for (int q = 0; q < ndir; ++q) {
            const int64_t off = G.dir[q].faces - c.d_faces.get();
            const int64_t d = dir_elems > 0 ? off / dir_elems : -1;
            if (off < 0 || d < 0 || d >= (int64_t)S.dir.size() || off - d * dir_elems != (sub ? H.fine.face_base : 0)) { found("launch_brick: the face block of direction %d of group %d starts at element %lld", q, gi, (long long)off); ok = false; break; }
            dirs[q] = (int)d;
            if (G.dir[q].w != S.dir[(size_t)d]->w) found("launch_brick: direction %d carries weight %a, the caller gave %a", (int)d, G.dir[q].w, S.dir[(size_t)d]->w);
            if (S.dir[(size_t)d]->izone != S.dir[(size_t)dirs[0]]->izone) found("launch_brick: group %d mixes izones %d and %d", gi, S.dir[(size_t)d]->izone, S.dir[(size_t)dirs[0]]->izone);
        }
        if (!ok) continue;
        if (!zone_map(S.dir[(size_t)dirs[0]]->izone, &Fr.zm)) { found("launch_brick: no frame for izone %d", S.dir[(size_t)dirs[0]]->izone); continue; }
        {
            const int slowest = Fr.layout, contiguous = Fr.layout == 2 ? 1 : 2; // layouts [ic][jc][kc], [jc][ic][kc], [kc][ic][jc]
            if (Fr.zm.src[slowest] != 0 || Fr.zm.src[contiguous] == 0) { found("launch_brick: group %d of izone %d marches through layout %d", gi, S.dir[(size_t)dirs[0]]->izone, Fr.layout); continue; }
            Fr.u_is_k = Fr.zm.src[contiguous] == 2;
            Fr.u_slot = Fr.u_is_k ? 2 : 1; Fr.v_slot = Fr.u_is_k ? 1 : 2;
        }
        const std::vector<ForestRegion> *boxes = sub || (size_t)gi >= H.regions.size() ? nullptr : &H.regions[(size_t)gi];

        const int cv0 = R * tv + 1, i0 = ti * chunk + 1, i1 = std::min(i0 + chunk - 1, n), sl = ti % ns;
        const int nrows = std::min(R, n - cv0 + 1);
        const bool has_u_in = tu > 0 || lane_lo > 0 || sub, has_u_out = 64 * (tu + 1) < n || lane_hi < 63 || sub;
        const bool has_v_in = tv > 0 || sub, has_v_out = R * (tv + 1) < n || sub;
        const bool has_i_in = ti > 0 || sub, has_i_out = i1 < n || sub;
        // element offsets inside a direction's face block (BrickLaunch, ftte_brick_rec.h)
        const int64_t u_out = lane_hi < 63 ? L.uqface_off + ((int64_t)((2 * box) * ns + sl) * chunk) * uw + ut * tv : ((int64_t)(tu * ns + sl) * chunk) * uw + ut * tv;
        const int64_t u_in = lane_lo > 0 ? L.uqface_off + ((int64_t)((2 * box + 1) * ns + sl) * chunk) * uw + ut * tv
                                         : ((int64_t)((tu > 0 ? tu - 1 : up / 64) * ns + sl) * chunk) * uw + ut * tv;
        const int64_t v_out = L.vface_off + ((int64_t)(tv * ns + sl) * chunk) * up + 64 * tu;
        const int64_t v_in = L.vface_off + ((int64_t)((tv > 0 ? tv - 1 : vp / R) * ns + sl) * chunk) * up + 64 * tu;
        const int64_t i_in = L.iface_off + ((int64_t)sl * vp + R * tv) * up + 64 * tu;
        const int64_t i_out = L.iface_off + ((int64_t)((ti + 1) % ns) * vp + R * tv) * up + 64 * tu;
        auto owned = [&](int lane) { return 64 * tu + lane + 1 <= n && lane >= lane_lo && lane <= lane_hi; };

        // the leaves of the brick's cells and of the cells one step behind it, once per task: [layer i0 .. i1 + 1][row cv0 .. cv0 + R][u0 .. u0 + 64]
        // (-1: a refined base cell, or no cell of the grid)
        const int u0 = 64 * tu + 1, Lv = R + 1, Lu = 65;
        leaf_of.assign((size_t)(i1 - i0 + 2) * Lv * Lu, -1);
        for (int i = i0; i <= std::min(i1 + 1, n); ++i)
            for (int v = cv0; v <= std::min(cv0 + R, n); ++v)
                for (int u = u0; u <= std::min(u0 + 64, n); ++u) {
                    int st[3];
                    Fr.storage(i, v, u, st);
                    leaf_of[((size_t)(i - i0) * Lv + (size_t)(v - cv0)) * Lu + (size_t)(u - u0)] = Fr.leaf(st);
                }
        // the segment whose incoming intensity is the ray that enters cell (i, v, u) through the face of segment `seg_slot`, or -1;
        // *out: the cell lies one step behind a sub-grid's last (side + 1 on one axis), and the segment is the one whose OUTGOING
        // intensity the sub-grid's last cell hands on through that face
        auto entering = [&](const model::DirOracle &O, int i, int v, int u, int seg_slot, bool *out) -> int64_t {
            *out = false;
            if (i > n || v > n || u > n) {
                if (!sub) return -1;
                int st[3];
                Fr.storage(std::min(i, n), std::min(v, n), std::min(u, n), st);
                const int32_t leaf = Fr.leaf(st);
                const auto it = leaf < 0 ? O.handed.end() : O.handed.find(3 * leaf + seg_slot);
                if (it == O.handed.end()) return -1;
                *out = true;
                return it->second;
            }
            const int32_t leaf = leaf_of[((size_t)(i - i0) * Lv + (size_t)(v - cv0)) * Lu + (size_t)(u - u0)];
            if (leaf < 0 || O.up[(size_t)(3 * leaf + seg_slot)] == AmrForest::kInactive) return -1;
            return 3 * (int64_t)leaf + seg_slot;
        };
        const size_t gn = (size_t)S.nnu;
        for (int q = 0; q < ndir; ++q) {
            const int d = dirs[q];
            const model::DirOracle &O = *S.dir[(size_t)d];
            double *F0 = G.dir[q].faces + (int64_t)L.nu0 * L.face_stride; // the launch's first frequency group
            // an element the kernel reads, in every group of the launch: it holds the oracle's value where the oracle has one
            auto reads = [&](int64_t e, int64_t seg, const char *what, int i, int v, int u) {
                for (int slot = 0; slot < L.nnu; ++slot) {
                    const double *at = F0 + (int64_t)slot * L.face_stride + e;
                    if (seg < 0) (void)touch(at);
                    else differs(at, O.Iin[(size_t)seg * gn + (size_t)(L.nu0 + slot)], what, d, L.nu0 + slot, i, v, u);
                }
            };
            // an element the kernel writes: the oracle's value, or a ray of no cell
            auto writes = [&](int64_t e, int64_t seg, bool out) {
                for (int slot = 0; slot < L.nnu; ++slot)
                    F0[(int64_t)slot * L.face_stride + e] = seg < 0 ? junk : (out ? O.Iout : O.Iin)[(size_t)seg * gn + (size_t)(L.nu0 + slot)];
            };
            bool out = false;
            // ---- the rays from the chunk below
            if (has_i_in)
                for (int r = 0; r < R; ++r)
                    for (int lane = 0; lane < 64; ++lane) {
                        const int v = cv0 + r, u = u0 + lane;
                        reads(i_in + (int64_t)r * up + lane, owned(lane) && v <= n ? entering(O, i0, v, u, 0, &out) : -1, "the ray from the chunk below", i0, v, u);
                    }
            for (int i = i0; i <= i1; ++i) {
                const int il = i - i0;
                const int rc = G.dir[q].layers[i - 1].info & 7;
                const bool hu = has_u(rc), hv = has_v(rc);
                {   // the layer's class against the oracle's pattern of the first cell the task owns
                    const int32_t leaf = leaf_of[((size_t)il * Lv) * Lu + (size_t)std::min(n - u0, lane_lo)];
                    if (leaf >= 0 && ((O.up[(size_t)(3 * leaf + Fr.u_slot)] != AmrForest::kInactive) != hu || (O.up[(size_t)(3 * leaf + Fr.v_slot)] != AmrForest::kInactive) != hv))
                        found("launch_brick: layer %d of direction %d has class %d, the oracle's cell has %s u piece and %s v piece", i, d, rc,
                              O.up[(size_t)(3 * leaf + Fr.u_slot)] != AmrForest::kInactive ? "a" : "no", O.up[(size_t)(3 * leaf + Fr.v_slot)] != AmrForest::kInactive ? "a" : "no");
                }
                if (hu)
                    for (int r = 0; r < R; ++r) {
                        const int v = cv0 + r;
                        if (has_u_in) { // what the first owned lane takes from the left
                            const int u = u0 + lane_lo;
                            reads(u_in + (int64_t)il * uw + r, v <= n && u <= n ? entering(O, i, v, u, Fr.u_slot, &out) : -1, "the ray from the left", i, v, u);
                        }
                        if (has_u_out) { // what the last owned lane hands to the right
                            const int64_t seg = v <= n && u0 + lane_hi <= n ? entering(O, i, v, u0 + lane_hi + 1, Fr.u_slot, &out) : -1;
                            writes(u_out + (int64_t)il * uw + r, seg, out);
                        }
                    }
                if (hv)
                    for (int lane = 0; lane < 64; ++lane) {
                        const int u = u0 + lane;
                        if (has_v_in) reads(v_in + (int64_t)il * up + lane, owned(lane) && cv0 <= n ? entering(O, i, cv0, u, Fr.v_slot, &out) : -1, "the ray from below", i, cv0, u);
                        if (has_v_out && (!masked || owned(lane))) {
                            const int64_t seg = u <= n && cv0 + R - 1 <= n ? entering(O, i, cv0 + R, u, Fr.v_slot, &out) : -1;
                            writes(v_out + (int64_t)il * up + lane, seg, out);
                        }
                    }
            }
            // ---- the rays for the chunk above
            if (has_i_out)
                for (int r = 0; r < R; ++r)
                    for (int lane = 0; lane < 64; ++lane) {
                        if (masked && !owned(lane)) continue;
                        const int v = cv0 + r, u = u0 + lane;
                        const int64_t seg = v <= n && u <= n ? entering(O, i1 + 1, v, u, 0, &out) : -1;
                        writes(i_out + (int64_t)r * up + lane, seg, out);
                    }
        }
        // ---- the accumulator: the cell means of the group's directions, in the order the layer takes them
        for (int slot = 0; slot < L.nnu; ++slot) (void)touch(L.uvb + L.nu0 + slot);
        for (int i = i0; i <= i1; ++i) {
            const int p0 = (ndir - (i - 1) % ndir) % ndir;
            for (int r = 0; r < nrows; ++r)
                for (int lane = 0; lane < 64; ++lane) {
                    if (!owned(lane)) continue;
                    const int v = cv0 + r, u = u0 + lane;
                    int st[3];
                    Fr.storage(i, v, u, st);
                    const int64_t at = G.org + (int64_t)i * G.si + (int64_t)v * G.sv + (G.su < 0 ? n + 1 - u : u);
                    if (at != Fr.element(st)) {
                        found("launch_brick: group %d puts cell (i %d, v %d, u %d) at element %lld of its array, its frame puts it at %lld", gi, i, v, u, (long long)at, (long long)Fr.element(st));
                        continue; // (no access: it may lie anywhere)
                    }
                    const int32_t leaf = leaf_of[((size_t)(i - i0) * Lv + (size_t)r) * Lu + (size_t)lane];
                    if (Fr.fine) { // the fine block's own map from its cells to the leaves, as the merge reads it
                        const int64_t cell = ((int64_t)(st[0] - 1) * n + (st[1] - 1)) * n + (st[2] - 1);
                        if (c.hdev.leaf_of_fine[cell] != leaf) found("launch_brick: fine cell %lld is leaf %d of the tree, the plan's map says %d", (long long)cell, leaf, c.hdev.leaf_of_fine[cell]);
                    }
                    bool inside = false;
                    if (boxes && leaf >= 0) {
                        const int j = Fr.u_is_k ? v : u, k = Fr.u_is_k ? u : v;
                        for (const ForestRegion &B : *boxes) inside = inside || B.contains(i, j, k);
                        if (inside) found("launch_brick: task %d of group %d owns cell (i %d, v %d, u %d) inside the group's box", t, gi, i, v, u);
                    }
                    for (int slot = 0; slot < L.nnu; ++slot) {
                        const int nu = L.nu0 + slot;
                        (void)touch(G.kappa + (int64_t)nu * L.group_stride + at);
                        if (L.emit) (void)touch(G.emis + (int64_t)nu * L.group_stride + at);
                        double *J = G.J + (int64_t)nu * L.group_stride + at;
                        const double before = accumulate ? touch(J) : 0.0;
                        if (leaf < 0 || inside) continue; // a refined base cell: the merge skips it
                        double Jacc = 0.0;
                        for (int j = 0; j < ndir; ++j) Jacc += S.dir[(size_t)dirs[(p0 + j) % ndir]]->cell[(size_t)leaf * gn + (size_t)nu];
                        *J = accumulate ? before + Jacc : Jacc;
                    }
                }
        }
    }
    return 0;
}

} // namespace ftte
