// brick_deal (ftte_brick_rec.h) on the CPU: which (task, frequency slot) pair each workgroup of a stage launch sweeps.
// For nnu = 1..16, run lengths 0, 1, 4, 16 and task counts from 1 to 1000:
//   every (task, slot) pair is swept by exactly one workgroup;
//   for a run length >= 1, among the workgroups of one class `work % kXcds` (one XCD under round-robin placement) the counts of
//   the slots differ by at most the run length;
//   run length 0 is slot = work % nnu, task = work / nnu.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "ftte_brick_rec.h"

using namespace ftte;

static int failures = 0;
#define CHECK(x) do { if (!(x)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #x); ++failures; } } while (0)

static void check(unsigned nnu, unsigned deal, unsigned ntasks)
{
    std::vector<int> seen((size_t)ntasks * nnu, 0);
    std::vector<long> count((size_t)kXcds * nnu, 0);
    for (unsigned work = 0; work < ntasks * nnu; ++work) {
        const BrickWork W = brick_deal(work, nnu, deal);
        if (W.task >= ntasks || W.slot >= nnu) { std::printf("nnu %u deal %u ntasks %u: workgroup %u -> task %u slot %u\n", nnu, deal, ntasks, work, W.task, W.slot); ++failures; return; }
        ++seen[(size_t)W.task * nnu + W.slot];
        ++count[(size_t)(work % kXcds) * nnu + W.slot];
        if (!deal) CHECK(W.slot == work % nnu && W.task == work / nnu);
    }
    for (size_t k = 0; k < seen.size(); ++k)
        if (seen[k] != 1) { std::printf("nnu %u deal %u ntasks %u: task %zu slot %zu swept %d times\n", nnu, deal, ntasks, k / nnu, k % nnu, seen[k]); ++failures; return; }
    if (!deal) return;
    for (unsigned x = 0; x < kXcds; ++x) {
        long lo = count[(size_t)x * nnu], hi = lo;
        for (unsigned s = 1; s < nnu; ++s) {
            const long v = count[(size_t)x * nnu + s];
            lo = v < lo ? v : lo; hi = v > hi ? v : hi;
        }
        if (hi - lo > (long)deal) { std::printf("nnu %u deal %u ntasks %u: class %u sweeps a slot %ld times and another %ld times\n", nnu, deal, ntasks, x, lo, hi); ++failures; }
    }
}

int main()
{
    const unsigned deals[] = {0, 1, 4, 16}, tasks[] = {1, 2, 7, 8, 64, 331, 1000};
    for (unsigned nnu = 1; nnu <= 16; ++nnu)
        for (unsigned deal : deals)
            for (unsigned ntasks : tasks) check(nnu, deal, ntasks);
    // the parent's placement, which the deal is there to break up: with four groups a slot stays on two classes
    {
        long on_class[kXcds] = {};
        for (unsigned work = 0; work < 4 * 1000; ++work)
            if (brick_deal(work, 4, 0).slot == 0) ++on_class[work % kXcds];
        CHECK(on_class[0] == 500 && on_class[4] == 500 && on_class[1] + on_class[2] + on_class[3] + on_class[5] + on_class[6] + on_class[7] == 0);
    }
    if (failures) return 1;
    std::printf("brick deal: ok\n");
    return 0;
}
