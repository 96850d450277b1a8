// The host side of the sweeps of a refined cell array -- forest_sweep (ftte_sweeps.cpp) and hybrid_sweep (ftte_hybrid.cpp) with
// everything they call: the planners, prepare_forests, the batches, passes and fused levels, the scratch slots, the face blocks, the
// group records, the cell-major copies, the merges -- run against a checked model of the device (tests/host/device_model.cpp) and
// a stub of the HIP runtime (tests/host/stub), under the address and undefined-behaviour sanitizers with leak detection.
//
// Per tree the program evaluates every direction with a loop of its own over build_forest without regions (the oracle), then
// sweeps on ONE context, call after call, so that every call finds the buffers the one before left.  Before a sweep the face block
// and the segment scratch are filled with a signalling NaN; fresh allocations come filled with 0xff bytes (another NaN,
// __asan_default_options below): an element read before anything wrote it fails a bitwise comparison.  After a sweep J is compared
// with the oracle (one direction: bit for bit; several: 64 eps relative, the rounding of the sum), what the oracle brick found is
// required to be nothing, and the forests' tables are checked property by property.  Three seeded faults prove the checks can fail.
#include <array>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <set>
#include <thread>

#include <sys/wait.h>
#include <unistd.h>

#include "device_model.h"

using namespace ftte;

extern "C" const char *__asan_default_options() { return "malloc_fill_byte=255:max_malloc_fill_size=2147483647"; }

#define CHECK(cond)                                                                                                \
    do {                                                                                                           \
        if (!(cond)) { std::fprintf(stderr, "ERROR %s:%d (%s): %s\n", __FILE__, __LINE__, g_case.c_str(), #cond); std::exit(1); } \
    } while (0)
static std::string g_case;

static int g_fail_code = 0; // what the last failure was refused with; its text is in the context
namespace ftte {
std::string g_create_error;
int fail(ftte_ctx *c, int code, const std::string &msg)
{
    g_fail_code = code;
    if (c) c->err = msg;
    else g_create_error = msg;
    return code;
}
} // namespace ftte

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

struct Dirs { std::vector<double> phi, theta, w; };
// one direction per izone: the first pixel of each at HEALPix level 3
static Dirs one_per_izone()
{
    Dirs D;
    D.phi.assign(24, 0); D.theta.assign(24, 0); D.w.assign(24, 1.0 / 24);
    bool have[25] = {};
    for (int64_t ipix = 0; ipix < 192; ++ipix) {
        double p, t, fp, ft;
        int izone = 0;
        CHECK(pix2ang_nest(4, ipix, &p, &t) == 0 && fold_direction(p, t, &fp, &ft, &izone) == 0 && izone >= 1 && izone <= 24);
        if (!have[izone]) { have[izone] = true; D.phi[(size_t)izone - 1] = p; D.theta[(size_t)izone - 1] = t; }
    }
    for (int z = 1; z <= 24; ++z) CHECK(have[z]);
    return D;
}

static const ftte_consts K = FTTE_CONSTS_INIT;

// ---- the oracle: the whole tree, direction by direction, depth by depth (the loop of forest_check.cpp, with the emission forms)
struct Medium { int nnu = 0, emit = 0; std::vector<double> kappa, emis, uvb; };
static std::vector<model::DirOracle> evaluate(const AmrTree &tree, double box, const Medium &M, const Dirs &D, const std::vector<uint8_t> &in_block)
{
    const int ndir = (int)D.phi.size(), nnu = M.nnu;
    const int64_t ncell = tree.ncell;
    std::vector<model::DirOracle> out((size_t)ndir);
    std::vector<int> status((size_t)ndir, 0);
    auto one = [&](int d) {
        model::DirOracle &O = out[(size_t)d];
        double p, t;
        if (fold_direction(D.phi[(size_t)d], D.theta[(size_t)d], &p, &t, &O.izone)) { status[(size_t)d] = 1; return; }
        AmrForest F;
        std::string err;
        if (build_forest(tree, p, t, O.izone, box, &F, &err)) { status[(size_t)d] = 2; return; }
        O.w = D.w[(size_t)d];
        O.up = F.up;
        O.Iin.assign((size_t)3 * ncell * nnu, 0.0); O.Iout.assign((size_t)3 * ncell * nnu, 0.0); O.mean.assign((size_t)3 * ncell * nnu, 0.0);
        for (size_t depth = 0; depth + 1 < F.depth_off.size(); ++depth)
            for (int64_t e = F.depth_off[depth]; e < F.depth_off[depth + 1]; ++e) {
                const int seg = F.order[(size_t)e];
                for (int g = 0; g < nnu; ++g) {
                    double I;
                    if (F.up[(size_t)seg] < 0) I = M.uvb[(size_t)g];
                    else {
                        I = O.Iout[(size_t)F.up[(size_t)seg] * nnu + g];
                        if (F.up2[(size_t)seg] >= 0) I = 0.5 * (I + O.Iout[(size_t)F.up2[(size_t)seg] * nnu + g]);
                    }
                    O.Iin[(size_t)seg * nnu + g] = I;
                    const double tau = M.kappa[(size_t)g * ncell + seg / 3] * F.dpath[(size_t)seg];
                    double m;
                    if (M.emit == 0) m = ftte_segment(&K, &I, tau);
                    else if (M.emit == 2) m = ftte_segment_source(&K, K.c[9], &I, tau, M.emis[(size_t)g * ncell + seg / 3]);
                    else m = ftte_segment_emit(&K, &I, tau, M.emis[(size_t)g * ncell + seg / 3], 0.0);
                    O.Iout[(size_t)seg * nnu + g] = I;
                    O.mean[(size_t)seg * nnu + g] = m;
                }
                // what a leaf of a fine block hands to a leaf outside it
                const int32_t up = F.up[(size_t)seg];
                if (!in_block.empty() && up >= 0 && F.up2[(size_t)seg] < 0 && in_block[(size_t)(up / 3)] && !in_block[(size_t)(seg / 3)]) O.handed[3 * (up / 3) + seg % 3] = up;
            }
        O.cell.resize((size_t)ncell * nnu);
        for (int64_t q = 0; q < ncell; ++q)
            for (int g = 0; g < nnu; ++g) {
                const size_t m = (size_t)(3 * q) * nnu + g;
                double acc = O.mean[m];
                int nseg = 1;
                if (F.up[(size_t)(3 * q + 1)] != AmrForest::kInactive) { acc += O.mean[m + nnu]; ++nseg; }
                if (F.up[(size_t)(3 * q + 2)] != AmrForest::kInactive) { acc += O.mean[m + 2 * (size_t)nnu]; ++nseg; }
                O.cell[(size_t)q * nnu + g] = ftte_cell_mean(acc, nseg, O.w);
            }
    };
    for (int d0 = 0; d0 < ndir; d0 += 8) {
        std::vector<std::thread> pool;
        for (int d = d0; d < std::min(ndir, d0 + 8); ++d) pool.emplace_back(one, d);
        for (auto &th : pool) th.join();
    }
    for (int s : status) CHECK(s == 0);
    return out;
}

// ---- a context as ftte_set_grid and ftte_set_opacity leave it
struct Sweeper {
    ftte_ctx *c = nullptr;
    DeviceBuffer<double> J_dev;
    std::vector<double> J;
    const Dirs *D = nullptr;
    const std::vector<model::DirOracle> *oracle = nullptr;
    const Medium *M = nullptr;
    std::vector<std::string> ran;

    void create(int n, const std::vector<int32_t> &level, const Medium &Md)
    {
        c = new ftte_ctx;
        CHECK(c->stream.create(hipStreamDefault) == hipSuccess);
        AmrTree tree;
        CHECK(tree.build(n, (int64_t)level.size(), level.data()).empty());
        c->leaf_level.assign(level.begin(), level.end());
        c->n = n; c->ncell = (int64_t)level.size(); c->box = 1.0; c->grid_set = true;
        c->kappa.invalidate();
        c->tree = std::move(tree);
        M = &Md;
        CHECK(ensure_kappa(c, Md.nnu) == FTTE_OK);
        CHECK(upload(c, c->kappa.source(), Md.kappa.data(), sizeof(double) * Md.kappa.size()) == FTTE_OK);
        c->nnu = Md.nnu;
        c->kappa.set();
        CHECK(J_dev.reserve((size_t)Md.nnu * (size_t)c->ncell) == hipSuccess);
        J.resize((size_t)Md.nnu * (size_t)c->ncell);
    }
    void set_medium(const Medium &Md) // the emissivity or source function of another oracle (as set_emission of ftte_api.cpp)
    {
        M = &Md;
        CHECK(wait_sweep(c) == FTTE_OK);
        if (!Md.emit) { c->emit_mode = 0; return; }
        CHECK(c->emis.reserve_source(c->kappa.capacity()) == hipSuccess);
        CHECK(hipMemcpy(c->emis.source(), Md.emis.data(), sizeof(double) * Md.emis.size(), hipMemcpyHostToDevice) == hipSuccess);
        c->emit_mode = Md.emit;
        c->emis.set();
    }
    void option(const char *key, int value) // ftte_set_option
    {
        std::string why;
        const OptionSet how = set(c->opt, key, value, &why);
        CHECK(how != OptionSet::refused);
        if (how == OptionSet::stored_invalidate) { c->plan.valid = c->bplan.valid = false; c->hplan.invalidate(); }
    }
    void destroy() { CHECK(hipStreamSynchronize(c->stream) == hipSuccess); delete c; c = nullptr; J_dev.reset(); }
};

// ---- the forests' tables, property by property.  Each returns what is wrong, or "" (the seeded faults need an answer, not an exit)
// the order of the records and the rays across the boxes' surfaces; listed[] grows depth by depth
static std::string order_and_exports(const ForestTables &T, int64_t nseg_all, int64_t base_elems, int64_t fine_base, int64_t fine_elems)
{
    char buf[256];
    auto bad = [&](const char *what, long long a, long long b) { std::snprintf(buf, sizeof buf, "%s (%lld, %lld)", what, a, b); return std::string(buf); };
    const int64_t ndepth = (int64_t)T.depth_off.size() - 1;
    std::vector<int32_t> listed((size_t)nseg_all, -1), pass_of_depth((size_t)std::max<int64_t>(ndepth, 1), 0);
    if (!T.pass_first.empty())
        for (size_t p = 0; p + 1 < T.pass_first.size(); ++p) for (int32_t k = T.pass_first[p]; k < T.pass_first[p + 1]; ++k) pass_of_depth[(size_t)k] = (int32_t)p;
    for (int64_t k = 0; k < ndepth; ++k) {
        for (int64_t e = T.depth_off[(size_t)k]; e < T.depth_off[(size_t)k + 1]; ++e) {
            const SegRec &R = T.rec[e];
            for (int32_t u : {R.up, R.up2})
                if (u >= 0 && (listed[(size_t)u] < 0 || listed[(size_t)u] >= k)) return bad("an upstream segment is not listed at a strictly earlier depth", R.seg, u);
        }
        for (int64_t e = T.depth_off[(size_t)k]; e < T.depth_off[(size_t)k + 1]; ++e) {
            if (listed[(size_t)T.rec[e].seg] >= 0) return bad("a segment listed twice", T.rec[e].seg, 0);
            listed[(size_t)T.rec[e].seg] = (int32_t)k;
        }
    }
    std::set<int32_t> export_at, fine_at;
    for (int64_t x = 0; x < T.nexports; ++x) {
        const AmrExport &X = T.exports[x];
        if (X.seg < 0 || X.seg >= nseg_all || listed[(size_t)X.seg] < 0) return bad("an export of a segment that is not listed", X.seg, 0);
        size_t pass = 0;
        if (!T.export_first.empty()) while (pass + 2 < T.export_first.size() && x >= T.export_first[pass + 1]) ++pass;
        if (pass_of_depth[(size_t)listed[(size_t)X.seg]] > (int32_t)pass) return bad("an export before its segment's pass", X.seg, (long long)pass);
        if (X.at < 0 || X.at >= base_elems) return bad("an export outside the base bricks' part of the face block", X.at, base_elems);
        if (!export_at.insert(X.at).second) return bad("two exports share a face element", X.at, 0);
    }
    for (int64_t x = 0; x < T.nimports; ++x) {
        const AmrImport &X = T.imports[x];
        if (X.up >= nseg_all || X.up2 >= nseg_all || (X.up >= 0 && listed[(size_t)X.up] < 0) || (X.up2 >= 0 && listed[(size_t)X.up2] < 0)) return bad("a fine import of a segment that is not listed", X.up, X.up2);
        if (X.at < fine_base || X.at >= fine_base + fine_elems) return bad("a fine import outside the fine bricks' part of the face block", X.at, fine_base);
        if (!fine_at.insert(X.at).second) return bad("two fine imports share a face element", X.at, 0);
    }
    return std::string();
}
static std::string tables_wrong(const ForestTables &T, int64_t nseg_all, int64_t base_elems, int64_t fine_base, int64_t fine_elems)
{
    // (what would send the walk of order_and_exports out of range is refused first)
    char buf[256];
    if (T.depth_off.empty() || T.depth_off[0] != 0) return "depth_off does not start at 0";
    for (size_t k = 0; k + 1 < T.depth_off.size(); ++k) if (T.depth_off[k] > T.depth_off[k + 1]) return "depth_off is not monotone";
    const int64_t nrec = T.depth_off.back(), ndepth = (int64_t)T.depth_off.size() - 1;
    if ((int64_t)T.rec.capacity() != std::max<int64_t>(nrec, 1)) return "depth_off does not end at the record count";
    if (!T.pass_first.empty()) {
        if (T.pass_first[0] != 0 || T.pass_first.back() != ndepth) return "pass_first does not span the depths";
        for (size_t p = 0; p + 1 < T.pass_first.size(); ++p) if (T.pass_first[p] > T.pass_first[p + 1]) return "pass_first is not monotone";
    }
    if (!T.export_first.empty()) {
        if (T.export_first[0] != 0 || T.export_first.back() != T.nexports) return "export_first does not span the exports";
        for (size_t p = 0; p + 1 < T.export_first.size(); ++p) if (T.export_first[p] > T.export_first[p + 1]) return "export_first is not monotone";
    }
    if (T.nexports && (int64_t)T.exports.capacity() != T.nexports) return "the export count is not the table's";
    if (T.nimports && (int64_t)T.imports.capacity() != T.nimports) return "the import count is not the table's";
    const int64_t all_elems = fine_elems ? fine_base + fine_elems : base_elems;
    std::set<int32_t> import_at;
    for (int64_t e = 0; e < nrec; ++e) {
        const SegRec &R = T.rec[e];
        if (R.seg < 0 || R.seg >= nseg_all || R.up >= nseg_all || R.up2 >= nseg_all) { std::snprintf(buf, sizeof buf, "record %lld names a segment outside the scratch (%d, %d, %d of %lld)", (long long)e, R.seg, R.up, R.up2, (long long)nseg_all); return buf; }
        if (R.up != AmrForest::kImport) continue;
        if (R.at < 0 || R.at >= all_elems || (fine_elems && R.at >= base_elems && R.at < fine_base)) { std::snprintf(buf, sizeof buf, "record %lld imports from element %d outside the direction's face block", (long long)e, R.at); return buf; }
        if (!import_at.insert(R.at).second) { std::snprintf(buf, sizeof buf, "two imports share face element %d", R.at); return buf; }
    }
    return order_and_exports(T, nseg_all, base_elems, fine_base, fine_elems);
}

enum Path { kHybrid, kForest };

struct Outcome { int rc = 0; bool hybrid = false; long mismatches = 0; std::string first; std::string tables; };

// One sweep of directions `list` of D on the context, as ftte_diffuse_sweep_device dispatches it; J against the oracle
static Outcome sweep(Sweeper &S, const std::vector<int> &list)
{
    ftte_ctx *c = S.c;
    const int ndir = (int)list.size(), nnu = c->nnu;
    const int64_t ncell = c->ncell;
    std::vector<double> phi, theta, w;
    model::State &MS = model::state();
    MS.clear();
    MS.c = c; MS.nnu = nnu; MS.dir.clear();
    for (int d : list) { phi.push_back(S.D->phi[(size_t)d]); theta.push_back(S.D->theta[(size_t)d]); w.push_back(S.D->w[(size_t)d]); MS.dir.push_back(&(*S.oracle)[(size_t)d]); }
    // poison: every face element and every scratch element there is, and J
    model::poison(c->d_faces.get(), c->d_faces.capacity());
    model::poison(c->fscratch.Iout.get(), c->fscratch.Iout.capacity());
    model::poison(c->fscratch.mean.get(), c->fscratch.mean.capacity());
    model::poison(S.J_dev.get(), S.J_dev.capacity());
    Outcome R;
    bool done = false;
    if (c->opt.hybrid.hybrid && c->tree.refined() && !c->opt.route.forest && ndir > 0)
        R.rc = hybrid_sweep(c, ndir, phi.data(), theta.data(), w.data(), S.M->uvb.data(), S.J_dev, c->stream, &done);
    if (!R.rc && !done) R.rc = forest_sweep(c, ndir, phi.data(), theta.data(), w.data(), S.M->uvb.data(), S.J_dev, c->stream);
    R.hybrid = done;
    if (R.rc) return R;
    CHECK(download(c, S.J.data(), S.J_dev, sizeof(double) * S.J.size()) == FTTE_OK && wait_sweep(c) == FTTE_OK);
    // ---- J
    const double rtol = ndir == 1 ? 0.0 : 64 * 2.220446049250313e-16;
    for (int g = 0; g < nnu; ++g)
        for (int64_t q = 0; q < ncell; ++q) {
            double want = 0.0;
            for (int d : list) want += (*S.oracle)[(size_t)d].cell[(size_t)q * nnu + g];
            const double got = S.J[(size_t)g * ncell + q];
            const bool same = ndir == 1 ? model::bits_of(got) == model::bits_of(want) : std::fabs(got - want) <= rtol * std::fabs(want);
            if (same) continue;
            if (!R.mismatches++) { char buf[200]; std::snprintf(buf, sizeof buf, "J of group %d, leaf %lld is %a, the oracle has %a", g, (long long)q, got, want); R.first = buf; }
        }
    if (MS.failures) { R.mismatches += MS.failures; if (R.first.empty()) R.first = MS.first; else R.first = MS.first + "; " + R.first; }
    // ---- the tables of whoever swept
    if (done) {
        const HybridPlan &H = c->hplan;
        const int64_t fine_elems = H.fine.active ? H.fine.plan.face_elems : 0;
        if (H.fine.active && H.fine.face_base != H.bricks.face_elems) R.tables = "the fine face block does not start behind the base bricks' rings";
        for (size_t d = 0; d < c->hdev.dirs.size() && R.tables.empty(); ++d) {
            R.tables = tables_wrong(c->hdev.dirs[d], 3 * c->hdev.ncells, H.bricks.face_elems, H.fine.face_base, fine_elems);
            if (!R.tables.empty()) R.tables = "direction " + std::to_string(d) + ": " + R.tables;
        }
    } else
        for (size_t d = 0; d < c->forests.dirs.size() && R.tables.empty(); ++d) {
            R.tables = tables_wrong(c->forests.dirs[d], 3 * ncell, 0, 0, 0);
            if (!R.tables.empty()) R.tables = "direction " + std::to_string(d) + ": " + R.tables;
        }
    return R;
}

// a sweep that has to come out clean on the path it is expected to take
static void clean(Sweeper &S, const std::vector<int> &list, Path want, const char *what)
{
    const std::string was = g_case;
    g_case += std::string(", ") + what;
    const auto t0 = std::chrono::steady_clock::now();
    const Outcome R = sweep(S, list);
    if (std::getenv("REFINED_SWEEP_TIMES")) std::printf("  %6.2f s  %s\n", std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count(), g_case.c_str());
    if (R.rc) std::fprintf(stderr, "ERROR %s: the sweep failed: %d %s\n", g_case.c_str(), R.rc, S.c->err.c_str());
    CHECK(R.rc == 0);
    if (R.mismatches) std::fprintf(stderr, "ERROR %s: %ld mismatches, the first: %s\n", g_case.c_str(), R.mismatches, R.first.c_str());
    if (!R.tables.empty()) std::fprintf(stderr, "ERROR %s: tables: %s\n", g_case.c_str(), R.tables.c_str());
    CHECK(R.mismatches == 0 && R.tables.empty());
    if (want == kHybrid) CHECK(R.hybrid && S.c->hplan.worthwhile);
    if (want == kForest) CHECK(!R.hybrid);
    if (R.hybrid) CHECK(model::state().brick_tasks > 0 && model::state().compared > 0);
    g_case = was;
}

struct TreeCase { const char *name; int n; std::set<Cell> blocks; int depth; int boxes, fine; bool several_passes; };

static const std::vector<int> kSingles = {0, 5, 10, 15, 20};

// whether a hybrid sweep with fewer directions resident than the call has goes through (ftte_hybrid.cpp: one pass, no slots side
// by side, no fine block) or is left to the forest path
static Path short_batch_path(const ftte_ctx *c)
{
    const HybridPlan &H = c->hplan;
    return (H.npass > 1 || (H.slots && H.nhalves > 1) || H.fine.active) ? kForest : kHybrid;
}

static void sequences(Sweeper &S, const TreeCase &T, const std::vector<int> &all, const char *form, bool only_a)
{
    ftte_ctx *c = S.c;
    auto tag = [&](const char *seq) { S.ran.push_back(std::string(T.name) + form + " nnu " + std::to_string(c->nnu) + " " + seq); };
    // (a) the order of the test that faulted on the device
    clean(S, all, kHybrid, "(a) 24 directions hybrid");
    CHECK(c->hplan.boxes() == T.boxes && c->hplan.fine_block() == T.fine && (c->hplan.npass > 1) == T.several_passes);
    // (the box cuts through a brick; rays cross its surface both ways; a fine block has bricks of its own and rays from the forest)
    CHECK(model::state().masked_tasks > 0 && model::state().exports > 0 && (T.fine != 0) == (model::state().sub_tasks > 0) && (T.fine != 0) == (model::state().imports > 0));
    for (int d : kSingles) clean(S, {d}, kHybrid, "(a) one direction hybrid");
    S.option("hybrid", 0);
    clean(S, all, kForest, "(a) 24 directions forest");
    for (int d : kSingles) clean(S, {d}, kForest, "(a) one direction forest");
    S.option("hybrid", 1);
    clean(S, all, kHybrid, "(a) 24 directions hybrid again");
    tag("(a)");
    if (only_a) return;
    // (b) pipelines
    for (int p : {1, 2, 4}) { S.option("pipelines", p); clean(S, all, kHybrid, "(b) pipelines"); }
    S.option("pipelines", 3);
    tag("(b)");
    // (c) a batch smaller than the direction count: a ragged last batch
    S.option("forest_batch", 5);
    S.option("hybrid", 0);
    clean(S, all, kForest, "(c) forest_batch 5 forest");
    S.option("hybrid", 1);
    {
        // (the scratch the forest path left holds every direction of the boxes: the option alone cuts the batch)
        const std::string was = g_case;
        g_case += ", (c) forest_batch 5 hybrid";
        const Outcome R = sweep(S, all);
        CHECK(R.rc == 0 && R.mismatches == 0 && R.tables.empty() && c->hplan.worthwhile);
        CHECK(R.hybrid == (short_batch_path(c) == kHybrid));
        g_case = was;
    }
    S.option("forest_batch", 0);
    tag("(c)");
    // (d) every level its own launch; whole passes in one
    S.option("forest_fuse", 0);
    clean(S, all, kHybrid, "(d) forest_fuse 0 hybrid");
    CHECK(model::state().fused == 0 && model::state().levels > 0);
    S.option("hybrid", 0);
    clean(S, {3}, kForest, "(d) forest_fuse 0 forest");
    S.option("hybrid", 1);
    S.option("forest_fuse", 1 << 24);
    clean(S, all, kHybrid, "(d) forest_fuse 2^24 hybrid");
    CHECK(model::state().fused > 0 && model::state().levels == 0);
    S.option("hybrid", 0);
    clean(S, {3}, kForest, "(d) forest_fuse 2^24 forest");
    S.option("hybrid", 1);
    S.option("forest_fuse", 4096);
    tag("(d)");
    // (e) little free memory: the batch is cut; the second scratch array cannot be had: a clean failure or smaller batches
    {
        const int nnu = c->nnu;
        const size_t forest_dir = (size_t)3 * (size_t)c->ncell * nnu;
        S.option("hybrid", 0);
        c->fscratch.drop();
        stub().free_bytes = (size_t)((double)(7 * 2 * sizeof(double) * forest_dir) / 0.9) + 64; // seven directions
        clean(S, all, kForest, "(e) free memory for seven directions, forest");
        CHECK(c->fscratch.capacity() == 7 * forest_dir);
        c->fscratch.drop();
        stub().fail_countdown = 2; // the forests are resident: the scratch arrays are the call's first two allocations
        clean(S, all, kForest, "(e) the second scratch array fails once, forest");
        CHECK(stub().fail_countdown == 0 && !stub().fail_next && c->fscratch.capacity() == 4 * forest_dir); // (seven halved)
        S.option("hybrid", 1);
        clean(S, all, kHybrid, "(e) warm-up hybrid"); // (plan and buffers resident again: the scratch is all a call allocates)
        const size_t hybrid_dir = (size_t)3 * (size_t)std::max<int64_t>(c->hdev.ncells, 1) * nnu;
        c->fscratch.drop();
        stub().free_bytes = (size_t)((double)(5 * 2 * sizeof(double) * hybrid_dir) / 0.6) + 64; // five directions
        {
            const std::string was = g_case;
            g_case += ", (e) free memory for five directions, hybrid";
            const Outcome R = sweep(S, all);
            CHECK(R.rc == 0 && R.mismatches == 0 && R.tables.empty());
            CHECK(R.hybrid == (short_batch_path(c) == kHybrid));
            g_case = was;
        }
        c->fscratch.drop();
        stub().free_bytes = (size_t)1 << 30;
        stub().fail_countdown = 2;
        {
            const Outcome R = sweep(S, all); // the hybrid path does not shrink: it fails cleanly, with nothing of the scratch left
            CHECK(stub().fail_countdown == 0 && !stub().fail_next);
            CHECK(R.rc == FTTE_ERR_NO_DEVICE && g_fail_code == FTTE_ERR_NO_DEVICE && !c->fscratch.Iout && !c->fscratch.mean && c->err.find("no room") != std::string::npos);
        }
        clean(S, all, kHybrid, "(e) the sweep after the failed one");
        tag("(e)");
    }
}

// ---- three seeded faults: each must be seen by a comparison (not by a sanitizer), each is undone, the sweep is clean again.
// expose = k: fault k stays in and the sweep goes through the check every clean sweep goes through, which ends the program
static void seeded_faults(Sweeper &S, const std::vector<int> &all, int expose = 0)
{
    ftte_ctx *c = S.c;
    clean(S, all, kHybrid, "before the seeded faults");
    const HybridPlan &H = c->hplan;
    auto exposed = [&](int k) {
        if (expose != k) return;
        clean(S, all, kHybrid, "a seeded fault");
        std::printf("seeded fault %d went unseen\n", k);
        std::exit(0);
    };
    // 1. an export's `at` moved by one element, still inside the block: a brick finds poison where its ray should wait
    if (expose == 0 || expose == 1) {
        int d = 0;
        while (d < 24 && c->hdev.dirs[(size_t)d].nexports == 0) ++d;
        CHECK(d < 24);
        AmrExport *X = c->hdev.dirs[(size_t)d].exports.get();
        const AmrExport was = X[0];
        X[0].at = was.at + 1 < H.bricks.face_elems ? was.at + 1 : was.at - 1;
        exposed(1);
        const Outcome R = sweep(S, all);
        X[0] = was;
        std::printf("  seeded fault 1 (an export moved by one element): %ld mismatches; %s\n", R.mismatches, R.first.c_str());
        CHECK(R.rc == 0 && model::state().failures > 0 && R.first.find("brick:") != std::string::npos);
        clean(S, all, kHybrid, "after seeded fault 1");
    }
    // 2. an `up` pointed at a segment of a later depth: the order property fails, and the read of its poisoned slot shows in J
    if (expose == 0 || expose == 2) {
        int d = 0;
        while (d < 24 && c->hdev.dirs[(size_t)d].depth_off.size() < 3) ++d;
        CHECK(d < 24);
        const ForestTables &T = c->hdev.dirs[(size_t)d];
        SegRec *rec = T.rec.get();
        const SegRec was = rec[0];
        rec[0].up = rec[T.depth_off.back() - 1].seg; rec[0].up2 = -1; // the first record of all takes the ray of the last
        exposed(2);
        const Outcome R = sweep(S, all);
        rec[0] = was;
        std::printf("  seeded fault 2 (an upstream segment of a later depth): %ld mismatches; %s; tables: %s\n", R.mismatches, R.first.c_str(), R.tables.c_str());
        CHECK(R.rc == 0 && R.mismatches > 0 && R.tables.find("strictly earlier") != std::string::npos);
        clean(S, all, kHybrid, "after seeded fault 2");
    }
    // 3. one brick task removed from its list -- a masked brick in front of a box: the forest imports poison
    if (expose == 0 || expose == 3) {
        const size_t nlists = (size_t)H.nhalves * H.nlist;
        const BrickTask *drop = nullptr;
        for (int h = 0; h < H.nhalves && !drop; ++h)
            for (size_t l = 0; l < (size_t)H.pass_at[(size_t)h][0] && !drop; ++l) {
                const size_t *off = &H.stage_off[nlists + (size_t)h * H.nlist];
                for (size_t q = off[l]; q < off[l + 1] && !drop; ++q)
                    if (((H.bricks.tasks[q].group >> kBrickLaneHiShift) & 63) < 63) drop = c->btables.tasks.get() + q; // its lanes end at a box
            }
        CHECK(drop);
        model::state().drop_task = drop;
        exposed(3);
        const Outcome R = sweep(S, all);
        model::state().drop_task = nullptr;
        std::printf("  seeded fault 3 (a brick task left out): %ld mismatches; %s\n", R.mismatches, R.first.c_str());
        CHECK(R.rc == 0 && R.mismatches > 0);
        clean(S, all, kHybrid, "after seeded fault 3");
    }
}

static Medium medium_for(int64_t ncell, int n, int nnu, int emit, uint64_t seed)
{
    Medium M;
    M.nnu = nnu; M.emit = emit;
    std::mt19937_64 rng(seed);
    std::uniform_real_distribution<double> decade(-3.0, -0.3), unit(0.1, 2.0);
    M.kappa.resize((size_t)nnu * (size_t)ncell);
    for (double &k : M.kappa) k = n * std::pow(10.0, decade(rng)); // optical depths of 0.001 .. 0.5 per base cell: thin and thick segments
    if (emit) { M.emis.resize(M.kappa.size()); for (size_t q = 0; q < M.emis.size(); ++q) M.emis[q] = emit == 2 ? unit(rng) : unit(rng) * M.kappa[q]; }
    const double uvb[3] = {1.0, 0.37, 2.5};
    M.uvb.assign(uvb, uvb + nnu);
    return M;
}

// form: the diagonal's launch lists by slot (1) or by phase (0); what: every sequence, sequence (a) alone, or the seeded faults and the emission forms
enum What { kSequences, kOnlyA, kExtras };
struct Job { size_t tree; int nnu; int form; What what; };

// One tree at one number of frequency groups on one context: the sequences, or the seeded faults and both emission forms
static std::vector<std::string> run_job(const Job &job, const TreeCase &T, const Dirs &D)
{
    std::vector<int> all(24);
    for (int d = 0; d < 24; ++d) all[(size_t)d] = d;
    const long base_live = stub().live;
    const int nnu = job.nnu;
    const std::vector<int32_t> level = levels_of(T.n, T.blocks, T.depth);
    AmrTree tree;
    CHECK(tree.build(T.n, (int64_t)level.size(), level.data()).empty());
    std::vector<uint8_t> in_block;
    if (T.fine) { // the leaves of the refined cube
        in_block.assign(level.size(), 0);
        for (size_t q = 0; q < level.size(); ++q) in_block[q] = level[q] == 1;
    }
    g_case = std::string(T.name) + (T.several_passes ? (job.form ? " slots" : " phases") : "") + ", nnu " + std::to_string(nnu);
    const std::string name = g_case;
    const Medium M = medium_for((int64_t)level.size(), T.n, nnu, 0, 1000 + 10 * job.tree + (uint64_t)nnu);
    const std::vector<model::DirOracle> oracle = evaluate(tree, 1.0, M, D, in_block);
    Sweeper S;
    S.D = &D; S.oracle = &oracle;
    S.create(T.n, level, M);
    S.option("chunk", 4);
    if (T.several_passes) S.option("hybrid_slots", job.form);
    if (job.what != kExtras) sequences(S, T, all, T.several_passes ? (job.form ? " slots" : " phases") : "", job.what == kOnlyA);
    if (T.several_passes) CHECK(S.c->hplan.slots == (job.form != 0));
    if (job.what == kExtras) {
        seeded_faults(S, all);
        S.ran.push_back(std::string(T.name) + " nnu 2 seeded faults");
        // both emission forms on this tree: a source function, then the reference's emissivity
        for (int emit : {2, 1}) {
            const Medium E = [&] { Medium X = medium_for((int64_t)level.size(), T.n, nnu, emit, 77 + (uint64_t)emit); X.kappa = M.kappa; return X; }();
            const std::vector<model::DirOracle> with = evaluate(tree, 1.0, E, D, in_block);
            S.oracle = &with;
            S.set_medium(E);
            g_case = std::string(T.name) + (emit == 2 ? ", source function" : ", emissivity");
            clean(S, all, kHybrid, "24 directions hybrid");
            clean(S, {7}, kHybrid, "one direction hybrid");
            S.option("hybrid", 0);
            clean(S, all, kForest, "24 directions forest");
            clean(S, {7}, kForest, "one direction forest");
            S.option("hybrid", 1);
            S.ran.push_back(std::string(T.name) + " nnu 2 " + (emit == 2 ? "source" : "eta"));
            S.set_medium(M);
            S.oracle = &oracle;
        }
    }
    model::state().c = nullptr;
    S.destroy();
    g_case = name;
    CHECK(stub().live == base_live);
    std::printf("%s: ok\n", g_case.c_str());
    std::fflush(stdout);
    return S.ran;
}

// refined_sweep_check [job | fault k | n128 corner]: every job, each in a process of its own (they share nothing; as many at a time
// as there are processors), or the one named; fault k: seeded fault k = 1, 2, 3 left in, which has to end the program with a failed
// check; n128 0 | 1: sequence (a) on the first or the last corner tree at the device test's own size
int main(int argc, char **argv)
{
    const Dirs D = one_per_izone();
    std::set<Cell> diagonal = cube({6, 6, 6}, 2, 2, 2);
    for (const Cell &x : cube({30, 30, 30}, 2, 2, 2)) diagonal.insert(x);
    for (const Cell &x : cube({54, 54, 54}, 2, 2, 2)) diagonal.insert(x);
    // the two trees of the device test that faulted, scaled down: a 3 x 2 x 3 patch in the first and in the last corner; a patch
    // against one face of the domain; case 2 of hybrid_plan_check.cpp; its three patches on the diagonal; its fully refined cube
    const std::vector<TreeCase> trees = {
        {"corner 0", 64, cube({0, 0, 0}, 3, 2, 3), 1, 1, 0, false},
        {"corner n - 3", 64, cube({61, 61, 61}, 3, 2, 3), 1, 1, 0, false},
        {"face 0", 64, cube({0, 20, 30}, 3, 2, 3), 1, 1, 0, false},
        {"face n - 3", 64, cube({61, 20, 30}, 3, 2, 3), 1, 1, 0, false},
        {"ragged two levels n = 72", 72, {{40, 41, 20}, {41, 41, 20}, {40, 42, 21}}, 2, 1, 0, false},
        {"diagonal", 64, diagonal, 1, 3, 0, true},
        {"refined 32^3 cube", 64, cube({8, 24, 12}, 32, 32, 32), 1, 1, 64, false},
    };
    // (the longest first.)  Every sequence with two frequency groups, the first corner tree with one and three as well.  The fully
    // refined tree has twice the leaves and takes twice as long as any other: it runs every sequence with ONE group and sequence
    // (a) with two, which is where a group's stride through the fine bricks' part of the face block enters.
    const std::vector<Job> jobs = {{6, 1, 1, kSequences}, {5, 2, 1, kSequences}, {5, 2, 0, kSequences}, {4, 2, 1, kSequences}, {0, 3, 1, kSequences}, {0, 2, 1, kSequences},
                                   {6, 2, 1, kOnlyA}, {1, 2, 1, kSequences}, {2, 2, 1, kSequences}, {3, 2, 1, kSequences}, {0, 2, 1, kExtras}, {0, 1, 1, kSequences}};
    auto line_of = [](const std::vector<std::string> &ran) { std::string l; for (const std::string &r : ran) l += " [" + r + "]"; return l; };
    if (argc > 2 && std::string(argv[1]) == "n128") { // the device test's own trees, n = 128, in its own order of calls: minutes and gigabytes, on request
        const int base = std::atoi(argv[2]) ? 128 - 3 : 0;
        const TreeCase T = {base ? "corner n - 3 at n = 128" : "corner 0 at n = 128", 128, cube({base, base, base}, 3, 2, 3), 1, 1, 0, false};
        std::printf("refined sweeps against the device model: ok:%s\n", line_of(run_job({0, 2, 1, kOnlyA}, T, D)).c_str());
        return 0;
    }
    if (argc > 2 && std::string(argv[1]) == "fault") { // the first corner tree with seeded fault argv[2] left in: ends with a failed check
        const TreeCase &T = trees[0];
        const std::vector<int32_t> level = levels_of(T.n, T.blocks, T.depth);
        AmrTree tree;
        CHECK(tree.build(T.n, (int64_t)level.size(), level.data()).empty());
        g_case = std::string(T.name) + ", seeded fault " + argv[2];
        const Medium M = medium_for((int64_t)level.size(), T.n, 2, 0, 1002);
        const std::vector<model::DirOracle> oracle = evaluate(tree, 1.0, M, D, {});
        Sweeper S;
        S.D = &D; S.oracle = &oracle;
        S.create(T.n, level, M);
        S.option("chunk", 4);
        std::vector<int> all(24);
        for (int d = 0; d < 24; ++d) all[(size_t)d] = d;
        seeded_faults(S, all, std::atoi(argv[2]));
        return 0;
    }
    if (argc > 1) {
        const size_t j = (size_t)std::atoi(argv[1]);
        CHECK(j < jobs.size());
        std::printf("refined sweeps against the device model: ok:%s\n", line_of(run_job(jobs[j], trees[jobs[j].tree], D)).c_str());
        return 0;
    }
    struct Child { pid_t pid; int fd; std::string said; bool done; };
    std::vector<Child> children;
    const size_t at_once = std::max(1u, std::min(16u, std::thread::hardware_concurrency()));
    size_t next = 0, running = 0, failed = 0;
    std::fflush(stdout);
    while (next < jobs.size() || running) {
        while (next < jobs.size() && running < at_once) {
            int fds[2];
            CHECK(pipe(fds) == 0);
            const pid_t pid = fork();
            CHECK(pid >= 0);
            if (pid == 0) {
                close(fds[0]);
                const std::string l = line_of(run_job(jobs[next], trees[jobs[next].tree], D));
                CHECK(write(fds[1], l.data(), l.size()) == (ssize_t)l.size());
                close(fds[1]);
                return 0; // (through exit: the leak check runs in every process)
            }
            close(fds[1]);
            children.push_back({pid, fds[0], std::string(), false});
            ++next; ++running;
        }
        int status = 0;
        const pid_t pid = wait(&status);
        CHECK(pid > 0);
        for (Child &C : children) {
            if (C.pid != pid) continue;
            char buf[4096];
            for (ssize_t got; (got = read(C.fd, buf, sizeof buf)) > 0;) C.said.append(buf, (size_t)got);
            close(C.fd);
            C.done = true;
            if (!WIFEXITED(status) || WEXITSTATUS(status) != 0) { ++failed; std::fprintf(stderr, "ERROR job %zu ended with status %d\n", (size_t)(&C - children.data()), status); }
        }
        --running;
    }
    CHECK(failed == 0);
    std::string line = "refined sweeps against the device model: ok:";
    for (const Child &C : children) line += C.said;
    std::printf("%s\n", line.c_str());
    return 0;
}
