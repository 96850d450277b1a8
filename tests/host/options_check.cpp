// The options of ftte_set_option (radiativetransfer_amd/csrc/ftte_options.h) against a literal copy of their contract, on a stub of
// the HIP runtime (tests/host/stub) under the address and undefined-behaviour sanitizers: the defaults, which values every option
// accepts, that an accepted value lands in the member named for it and nowhere else, that a refusal changes nothing and names the
// option, which options drop the plans, the table's shape, and unknown keys.  Values are read from the named members of Options,
// never through the table's accessor: a row wired to the wrong member fails here.
// With --names: the table's names, one per line (tests/test_options_host.py compares them with include/ftte.h).
#include <array>
#include <climits>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <set>
#include <string>
#include <vector>

#include "ftte_options.h"

using namespace ftte;

#define CHECK(cond)                                                                                                \
    do {                                                                                                           \
        if (!(cond)) { std::fprintf(stderr, "ERROR %s:%d: %s (option %s, value %d)\n", __FILE__, __LINE__, #cond, g_name, g_value); std::exit(1); } \
    } while (0)
static const char *g_name = "-";
static int g_value = 0;

// The contract: accepted are lo..hi, or where `only` is not empty exactly its values
struct Want { const char *name; int lo, hi; std::vector<int> only; int def; bool invalidates; };
static const std::vector<Want> kContract = {
    {"rows", 4, 16, {4, 8, 16}, 8, true},
    {"slots", 1, 16, {}, 8, true},
    {"waves", 2, 6, {}, 4, true},
    {"stack", 1, 8, {1, 2, 4, 8}, 1, true},
    {"engine", 0, 2, {}, 0, true},
    {"forest", 0, 1, {}, 0, true},
    {"ldspad", 0, 163840, {}, 0, true},
    {"chunk", 0, 4096, {}, 0, true},
    {"group", 0, 8, {}, 0, true},
    {"share", 0, 2, {}, 2, true},
    {"lanes", 1, 16, {}, 2, true},
    {"team", -1, 2, {-1, 0, 2}, -1, true},
    {"dataflow", 0, 3, {}, 0, true},
    {"queue_mix", 0, 2, {}, 0, true},
    {"brick_waves", 2, 4, {}, 4, true},
    {"pair_waves", 2, 4, {}, 4, true},
    {"atomic_acc", 0, 1, {}, 0, true},
    {"nu_deal", 0, 4096, {}, 16, false},
    {"ablate", 0, 63, {}, 0, true},
    {"tiled", 0, 2, {}, 0, true},
    {"merge_overlap", 0, 1, {}, 1, true},
    {"forest_fuse", 0, 16777216, {}, 4096, true},
    {"hybrid", 0, 1, {}, 1, true},
    {"hybrid_slots", 0, 2, {}, 1, true},
    {"graph", 0, 1, {}, 0, true},
    {"box_lanes", 1, 64, {1, 2, 4, 8, 16, 32, 64}, 1, true},
    {"forest_batch", 0, 65535, {}, 0, true},
    {"pipelines", 1, 4, {}, 3, true},
    {"fine_bricks", 0, 1, {}, 1, true},
    {"fine_chunk", 0, 4096, {}, 0, true},
};
constexpr size_t kCount = 30;

// every member of Options, by name, in the contract's order
using Values = std::array<int, kCount>;
static Values values(const Options &o)
{
    return {o.tile.rows, o.tile.slots, o.tile.waves, o.tile.stack, o.route.engine, o.route.forest, o.launch.lds_pad,
            o.brick.chunk, o.brick.group, o.brick.share, o.brick.lanes, o.brick.team, o.brick.dataflow, o.brick.queue_mix,
            o.launch.brick_waves, o.launch.pair_waves, o.launch.atomic_acc, o.launch.nu_deal, o.launch.ablate, o.launch.tiled,
            o.launch.merge_overlap, o.launch.forest_fuse,
            o.hybrid.hybrid, o.hybrid.slots, o.hybrid.graph, o.hybrid.lanes, o.hybrid.forest_batch, o.hybrid.pipelines,
            o.hybrid.fine_bricks, o.hybrid.fine_chunk};
}
// (Options is nothing but these: thirty ints)
static_assert(sizeof(Options) == kCount * sizeof(int), "a member of Options that values() does not list");

static bool wanted(const Want &w, int v)
{
    if (v < w.lo || v > w.hi) return false;
    if (w.only.empty()) return true;
    for (int a : w.only) if (a == v) return true;
    return false;
}

int main(int argc, char **argv)
{
    if (argc > 1 && !std::strcmp(argv[1], "--names")) {
        for (const OptionRow &row : kOptionTable) std::printf("%s\n", row.name);
        return 0;
    }
    // table shape
    std::set<std::string> names;
    for (const OptionRow &row : kOptionTable) names.insert(row.name);
    CHECK(sizeof kOptionTable / sizeof kOptionTable[0] == kCount && names.size() == kCount && kContract.size() == kCount);
    for (const Want &w : kContract) { g_name = w.name; CHECK(names.count(w.name) == 1); }

    // defaults
    const Values fresh = values(Options());
    for (size_t k = 0; k < kCount; ++k) { g_name = kContract[k].name; g_value = fresh[k]; CHECK(fresh[k] == kContract[k].def); }

    // accepted and refused values, from the defaults and from a state in which every option holds an accepted value other than
    // its default (so that a value stored into the wrong member, or a refusal that resets one, shows)
    Options moved;
    for (const Want &w : kContract) {
        const int v = w.only.empty() ? (w.def == w.hi ? w.lo : w.hi) : (w.def == w.only.back() ? w.only.front() : w.only.back());
        std::string why;
        g_name = w.name; g_value = v;
        CHECK(v != w.def && set(moved, w.name, v, &why) != OptionSet::refused);
    }
    const Options defaults;
    const Options *const starts[] = {&defaults, &moved};
    long accepted = 0, refused = 0;
    for (const Options *start : starts)
        for (size_t k = 0; k < kCount; ++k) {
            const Want &w = kContract[k];
            g_name = w.name;
            auto check = [&](int v) {
                g_value = v;
                Options o = *start;
                Values expect = values(o);
                std::string why;
                const OptionSet how = set(o, w.name, v, &why);
                if (wanted(w, v)) {
                    ++accepted;
                    expect[k] = v;
                    CHECK(how == (w.invalidates ? OptionSet::stored_invalidate : OptionSet::stored) && why.empty() && values(o) == expect);
                    // the value already there: stored again, and the plans go as they did
                    CHECK(set(o, w.name, v, &why) == how && why.empty());
                } else {
                    ++refused;
                    CHECK(how == OptionSet::refused && !why.empty() && why.compare(0, std::strlen(w.name), w.name) == 0);
                }
                CHECK(values(o) == expect);
            };
            check(INT_MIN);
            check(INT_MAX);
            // Every value of [lo - 2, hi + 2].  forest_fuse alone (0..2^24) is sampled: both ends with the two values beyond them,
            // every power of two with its neighbours, and every 4099th value in between; each of its 16.8 million values took this
            // program 18 s under the sanitizers (4 s without them)
            if (w.hi - w.lo <= 1 << 18) for (int v = w.lo - 2; v <= w.hi + 2; ++v) check(v);
            else {
                for (int v : {w.lo - 2, w.lo - 1, w.lo, w.lo + 1, w.hi - 1, w.hi, w.hi + 1, w.hi + 2}) check(v);
                for (int p = 1; p > 0 && p <= w.hi - w.lo; p *= 2) for (int v : {w.lo + p - 1, w.lo + p, w.lo + p + 1}) check(v);
                for (int v = w.lo; v <= w.hi - 4099; v += 4099) check(v);
            }
        }

    // unknown keys
    g_value = 1;
    for (const char *key : {"", "chun", "chunk ", "multi_reduce", "no such option"})
        for (const Options *start : starts) {
            g_name = key;
            Options o = *start;
            std::string why;
            CHECK(set(o, key, 1, &why) == OptionSet::refused && !why.empty() && values(o) == values(*start));
        }

    std::printf("options under the sanitizers: ok (%ld accepted, %ld refused)\n", accepted, refused);
    return 0;
}
