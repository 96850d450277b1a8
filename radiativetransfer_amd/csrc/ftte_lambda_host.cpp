// ftte_lambda_host.cpp -- the host side of the accelerated source iteration (include/ftte.h: ftte_lambda_diagonal, ftte_source_update_device):
// the per-direction tables of segment lengths the diagonal kernel reads, the leaves' places on their levels, and the entry points.
//
// Geometry.  After the izone rotation every cell of a layer along the march axis carries the same ray pattern (setPattern,
// equiSources.f90:1495-1534), and on a refined cell array every child of a sub-layer carries that sub-layer's pattern, one pattern
// tree per base layer (setRaysRefined, transportRoutinesModule.f90:150-187).  So a leaf of level l needs the record of sub-layer
// m in [0, n 2^l) of its level, m its position along the march axis on that level's grid (counted against the axis where the
// izone mirrors it): a table per (direction, level), no forest, box, pass or brick plan, and no sweep option matters.
#include "ftte_context.h"

using namespace ftte;

namespace {

LambdaRec record_of(const ftte_pattern &p, double cell)
{
    LambdaRec R;
    R.dpath[0] = cell * p.xy_len; // as the planners form it (plan_direction, leaf_segments)
    R.dpath[1] = p.xz_active ? cell * p.xz_len : 0.0;
    R.dpath[2] = p.yz_active ? cell * p.yz_len : 0.0;
    R.nseg = 1 + (p.xz_active ? 1 : 0) + (p.yz_active ? 1 : 0);
    R.pad_ = 0;
    return R;
}

// The leaves' levels and storage positions, and which sub-layers of each level hold a leaf at all (per storage axis)
int make_leaves(ftte_ctx *c)
{
    if (c->d_lambda_leaves && c->lambda_leaves_grid == c->n_grid_builds) return FTTE_OK;
    const AmrTree &T = c->tree;
    const int n = c->n, L = T.max_level;
    const size_t nnode = T.parent.size(), per_axis = (size_t)n * ((2u << L) - 1);
    std::vector<int32_t> pos(3 * nnode);
    std::vector<LambdaLeaf> leaves((size_t)c->ncell);
    c->lambda_used.assign(3 * per_axis, 0);
    for (size_t node = 0; node < nnode; ++node) {
        int32_t *p = &pos[3 * node];
        if (T.parent[node] < 0) {
            p[0] = (int32_t)(node / ((size_t)n * n)); p[1] = (int32_t)((node / (size_t)n) % (size_t)n); p[2] = (int32_t)(node % (size_t)n);
        }
        const int lv = T.level[node];
        if (T.child0[node] >= 0) {
            // the 8 children are contiguous, indexed 4a + 2b + c by their storage offsets (a, b, c); they come after their parent
            for (int ch = 0; ch < 8; ++ch) {
                int32_t *q = &pos[3 * ((size_t)T.child0[node] + (size_t)ch)];
                q[0] = 2 * p[0] + ((ch >> 2) & 1); q[1] = 2 * p[1] + ((ch >> 1) & 1); q[2] = 2 * p[2] + (ch & 1);
            }
        } else {
            LambdaLeaf &F = leaves[(size_t)T.leaf[node]];
            F.level = lv;
            const size_t off = (size_t)n * ((1u << lv) - 1);
            for (int a = 0; a < 3; ++a) { F.pos[a] = p[a]; c->lambda_used[(size_t)a * per_axis + off + (size_t)p[a]] = 1; }
        }
    }
    FTTE_HIP(c, c->d_lambda_leaves.reserve(leaves.size()));
    FTTE_HIP(c, hipMemcpy(c->d_lambda_leaves, leaves.data(), sizeof(LambdaLeaf) * leaves.size(), hipMemcpyHostToDevice));
    c->lambda_leaves_grid = c->n_grid_builds;
    return FTTE_OK;
}

// The tables of a direction list: per direction n records of level 0, 2 n of level 1, ... (stride records in all)
int make_tables(ftte_ctx *c, int ndir, const double *phi, const double *theta, const double *w, bool refined, int *stride_out)
{
    const int n = c->n, L = refined ? c->tree.max_level : 0;
    const size_t stride = (size_t)n * ((2u << L) - 1);
    std::vector<LambdaRec> table(stride * (size_t)std::max(ndir, 1));
    std::vector<LambdaDir> dirs((size_t)std::max(ndir, 1));
    std::vector<ftte_pattern> cur, next;
    std::vector<uint8_t> bad, bad_next;
    for (int d = 0; d < ndir; ++d) {
        double ph, th;
        int izone;
        const int rc = fold_direction(phi[d], theta[d], &ph, &th, &izone);
        if (rc) {
            char buf[160];
            std::snprintf(buf, sizeof buf, "direction %d (phi=%.17g, theta=%.17g) cannot be folded: %s", d, phi[d], theta[d],
                          rc == 1 ? "phi on a quadrant boundary" : rc == 2 ? "theta outside (-pi/2,0)u(0,pi/2)" : "tie between dominant axes");
            return fail(c, fold_status(rc), buf);
        }
        cur.resize((size_t)n);
        if (layer_patterns(n, ph, th, cur.data()))
            return fail(c, FTTE_ERR_PATTERN, "direction " + std::to_string(d) + ": ray pattern left the unit cell (setPattern consistency check)");
        ZoneMap zm;
        zone_map(izone, &zm);
        LambdaDir &D = dirs[(size_t)d];
        D.w = w[d];
        D.axis = 0;
        for (int a = 0; a < 3; ++a) if (zm.src[a] == 0) D.axis = a; // the storage axis the march runs along (rotate_indices)
        D.mirror = zm.mirror[D.axis] ? 1 : 0;
        LambdaRec *out = &table[stride * (size_t)d];
        double cell = c->box / (double)n; // cellSizeAbsoluteUnits, equiSources.f90:1570
        bad.assign((size_t)n, 0);
        for (int lv = 0;; ++lv) {
            const size_t side = cur.size();
            for (size_t m = 0; m < side; ++m) {
                if (!bad[m]) { out[m] = record_of(cur[m], cell); continue; }
                // a sub-layer whose pattern the reference would stop at: an error only where a leaf lies in it
                const size_t place = D.mirror ? side - 1 - m : m;
                if (c->lambda_used[(size_t)D.axis * stride + (size_t)(out - &table[stride * (size_t)d]) + place])
                    return fail(c, FTTE_ERR_PATTERN, "direction " + std::to_string(d) + ": ray pattern left the unit cell (sub-layer patterns of a refined cell)");
                out[m] = LambdaRec{{0.0, 0.0, 0.0}, 1, 0};
            }
            if (lv == L) break;
            next.resize(2 * side);
            bad_next.assign(2 * side, 0);
            for (size_t m = 0; m < side; ++m)
                if (bad[m] || sub_layer_patterns(cur[m], ph, th, &next[2 * m], &next[2 * m + 1])) bad_next[2 * m] = bad_next[2 * m + 1] = 1;
            out += side;
            cur.swap(next);
            bad.swap(bad_next);
            cell = cell / 2.0; // transport's recursion, transportRoutinesModule.f90:577-586
        }
    }
    FTTE_HIP(c, c->d_lambda_table.reserve(table.size()));
    FTTE_HIP(c, c->d_lambda_dirs.reserve(dirs.size()));
    FTTE_HIP(c, hipMemcpy(c->d_lambda_table, table.data(), sizeof(LambdaRec) * table.size(), hipMemcpyHostToDevice));
    FTTE_HIP(c, hipMemcpy(c->d_lambda_dirs, dirs.data(), sizeof(LambdaDir) * dirs.size(), hipMemcpyHostToDevice));
    *stride_out = (int)stride;
    return FTTE_OK;
}

} // namespace

extern "C" {

int ftte_lambda_diagonal_device(ftte_ctx *c, int ndir, const double *phi, const double *theta, const double *w, double *diag_dev,
                                void *stream_v)
{
    int rc = check_ready(c, true);
    if (rc) return rc;
    if (ndir < 0 || (ndir > 0 && (!phi || !theta || !w)) || !diag_dev) return fail(c, FTTE_ERR_ARG, "ftte_lambda_diagonal: bad argument");
    FTTE_HIP(c, hipSetDevice(c->device));
    hipStream_t stream = stream_v ? (hipStream_t)stream_v : c->stream;
    // whatever still reads the tables or writes the opacities has finished; the setters wait for this call in turn (mark_sweep)
    if ((rc = wait_sweep(c))) return rc;
    FTTE_HIP(c, hipStreamSynchronize(c->stream));
    const bool refined = c->tree.refined();
    if (refined) {
        if ((uint64_t)c->n << c->tree.max_level >= (1u << 30)) return fail(c, FTTE_ERR_UNSUPPORTED, "ftte_lambda_diagonal: more than 2^30 cells a side on the finest level");
        if ((rc = make_leaves(c))) return rc;
    }
    int stride = 0;
    if ((rc = make_tables(c, ndir, phi, theta, w, refined, &stride))) return rc;
    static const ftte_consts kMath = FTTE_CONSTS_INIT;
    LambdaLaunch L;
    L.kappa = c->kappa.source(); L.diag = diag_dev;
    L.table = c->d_lambda_table; L.dirs = c->d_lambda_dirs; L.leaves = refined ? c->d_lambda_leaves.get() : nullptr;
    L.ncell = c->ncell; L.n = c->n; L.nnu = c->nnu; L.ndir = ndir; L.stride = stride;
    L.K = kMath;
    if (launch_lambda_diagonal(L, refined, stream)) return fail(c, FTTE_ERR_NO_DEVICE, "ftte_lambda_diagonal: kernel launch failed");
    return mark_sweep(c, stream);
}

int ftte_lambda_diagonal(ftte_ctx *c, int ndir, const double *phi, const double *theta, const double *w, double *diag)
{
    int rc = check_ready(c, true);
    if (rc) return rc;
    if (!diag) return fail(c, FTTE_ERR_ARG, "ftte_lambda_diagonal: diag is NULL");
    FTTE_HIP(c, hipSetDevice(c->device));
    const size_t elems = (size_t)c->nnu * c->ncell;
    FTTE_HIP(c, c->d_lambda_host.reserve(elems));
    if ((rc = ftte_lambda_diagonal_device(c, ndir, phi, theta, w, c->d_lambda_host, nullptr))) return rc;
    if ((rc = download(c, diag, c->d_lambda_host, sizeof(double) * elems))) return rc;
    return wait_sweep(c);
}

int ftte_source_update_device(ftte_ctx *c, int nnu, double epsilon, const double *B_dev, int b_per_cell, const double *J_dev,
                              const double *diag_dev, double *S_dev, double *change, void *stream_v)
{
    int rc = check_ready(c, false);
    if (rc) return rc;
    if (nnu < 1 || !B_dev || !J_dev || !S_dev || !(epsilon >= 0.0 && epsilon <= 1.0)) return fail(c, FTTE_ERR_ARG, "ftte_source_update_device: bad argument");
    FTTE_HIP(c, hipSetDevice(c->device));
    hipStream_t stream = stream_v ? (hipStream_t)stream_v : c->stream;
    FTTE_HIP(c, c->d_update_stats.reserve(4));
    FTTE_HIP(c, c->h_update_stats.reserve(4));
    unsigned long long *h = c->h_update_stats;
    h[0] = ~0ull; h[1] = h[2] = h[3] = 0ull;
    FTTE_HIP(c, hipMemcpyAsync(c->d_update_stats, h, 4 * sizeof *h, hipMemcpyHostToDevice, stream));
    UpdateLaunch U;
    U.J = J_dev; U.B = B_dev; U.diag = diag_dev; U.S = S_dev;
    U.stats = c->d_update_stats;
    U.ncell = c->ncell; U.eps = epsilon; U.nnu = nnu; U.b_per_cell = b_per_cell ? 1 : 0;
    if (launch_source_update(U, stream)) return fail(c, FTTE_ERR_NO_DEVICE, "ftte_source_update_device: kernel launch failed");
    FTTE_HIP(c, hipMemcpyAsync(h, c->d_update_stats, 4 * sizeof *h, hipMemcpyDeviceToHost, stream));
    FTTE_HIP(c, hipStreamSynchronize(stream));
    if (h[0] != ~0ull) {
        char buf[224];
        std::snprintf(buf, sizeof buf, "ftte_source_update_device: 1 - (1 - epsilon) Lambda* is not positive in element %llu (group %llu, cell %llu; "
                      "the weights of the direction list sum to more than 1 / (1 - epsilon)?); S is unchanged", h[0], h[0] / (unsigned long long)c->ncell,
                      h[0] % (unsigned long long)c->ncell);
        return fail(c, FTTE_ERR_ARG, buf);
    }
    if (change) { std::memcpy(&change[0], &h[1], sizeof(double)); std::memcpy(&change[1], &h[2], sizeof(double)); }
    return FTTE_OK;
}

} // extern "C"
