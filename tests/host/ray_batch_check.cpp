// ftte::ray_batch_rays (radiativetransfer_amd/csrc/ftte_rays.h) against a stub of the HIP runtime (tests/host/stub), as a program of
// its own, with and without the sanitizers (tests/test_rays_host.py): the rule that keeps what a batch of rays holds -- per_segment
// bytes for every segment of its rays, three doubles of summaries per ray, nvel doubles of tau per ray where tau is staged -- under
// kSpectraWorkBytes.  Known values written out, the property over random counts, and with a file of rows
// "nvel stage_tau per_segment nray count_0 .. count_{nray-1}" the batches of each row on one line, for the tests' restatement of the
// rule (tests/_rays.py: batch_rays) to be held against.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "ftte_rays.h"

using namespace ftte;

#define CHECK(cond)                                                                                                \
    do {                                                                                                           \
        if (!(cond)) { std::fprintf(stderr, "ERROR %s:%d: %s\n", __FILE__, __LINE__, #cond); std::exit(1); }       \
    } while (0)

// what the tests' restatement takes as given
static_assert(kSpectraWorkBytes == (size_t)1 << 26, "the budget of a batch");
static_assert(kSpectraChunk == 512, "chunk");
static_assert(sizeof(ftte_spectra_seg) == 32 && kRaySegmentListBytes == 24, "a record, a list entry");

struct Lcg {
    uint64_t s;
    uint64_t next() { s = s * 6364136223846793005ull + 1442695040888963407ull; return s >> 11; }
};

static std::vector<int64_t> prefix(const std::vector<int64_t> &count)
{
    std::vector<int64_t> off(count.size() + 1, 0);
    for (size_t r = 0; r < count.size(); ++r) off[r + 1] = off[r] + count[r];
    return off;
}

static std::vector<int64_t> batches(const std::vector<int64_t> &off, int64_t nvel, bool stage, size_t per_segment)
{
    std::vector<int64_t> out;
    const int64_t nray = (int64_t)off.size() - 1;
    for (int64_t at = 0; at < nray;) {
        const int64_t m = ray_batch_rays(off.data(), nray, at, nvel, stage, per_segment);
        CHECK(m >= 1 && at + m <= nray);
        out.push_back(m);
        at += m;
    }
    return out;
}

int main(int argc, char **argv)
{
    if (argc > 1) {
        std::FILE *f = std::fopen(argv[1], "r");
        if (!f) { std::printf("cannot read %s\n", argv[1]); return 2; }
        long long nvel, per_segment, nray;
        int stage;
        while (std::fscanf(f, "%lld %d %lld %lld", &nvel, &stage, &per_segment, &nray) == 4) {
            std::vector<int64_t> count((size_t)nray);
            for (auto &c : count) { long long v; if (std::fscanf(f, "%lld", &v) != 1) return 2; c = v; }
            for (int64_t m : batches(prefix(count), nvel, stage != 0, (size_t)per_segment)) std::printf("%lld ", (long long)m);
            std::printf("\n");
        }
        std::fclose(f);
        return 0;
    }
    // 4 segments a ray, tau of 4096 pixels staged: (4 * 32 + 24 + 32768) bytes a ray -> 2038 rays
    CHECK((batches(prefix(std::vector<int64_t>(4608, 4)), 4096, true, 32) == std::vector<int64_t>{2038, 2038, 532}));
    // tau not staged: 152 bytes a ray, one batch
    CHECK((batches(prefix(std::vector<int64_t>(4608, 4)), 4096, false, 32) == std::vector<int64_t>{4608}));
    // one ray over the budget still gets a batch of its own, and its neighbours theirs
    CHECK((batches(prefix({10, 3000000, 10, 10}), 64, true, 32) == std::vector<int64_t>{1, 1, 2}));
    CHECK((batches(prefix({3000000}), 64, true, 32) == std::vector<int64_t>{1}));
    // the segment list: 24 bytes a segment and the ray's 24
    CHECK((batches(prefix(std::vector<int64_t>(3, 1000000)), 0, false, 24) == std::vector<int64_t>{2, 1}));
    // rays without segments cost their summaries alone
    CHECK((batches(prefix(std::vector<int64_t>(100000, 0)), 8, true, 32) == std::vector<int64_t>{100000}));
    const int64_t none[1] = {0};
    CHECK(ray_batch_rays(none, 0, 0, 64, true, 32) == 1 && ray_batch_rays(none, -3, 0, 64, true, 32) == 1);
    const std::vector<int64_t> two = prefix({5, 5});
    CHECK(ray_batch_rays(two.data(), 2, 2, 64, true, 32) == 1 && ray_batch_rays(two.data(), 2, -1, 64, true, 32) == 1 && ray_batch_rays(two.data(), 2, 1, -7, true, 32) == 1);

    Lcg r{20261021ull};
    int over = 0, whole = 0, cut = 0;
    for (int q = 0; q < 300; ++q) {
        const size_t nray = (size_t)(1 + r.next() % (q % 3 ? 20000 : 40));
        const int64_t nvel = (int64_t)(r.next() % (q % 5 ? 20000 : (1 << 24)));
        const bool stage = r.next() & 1;
        const size_t per_segment = q % 2 ? 32 : 24;
        const uint64_t most = q % 7 ? 3000 : 4000000;
        std::vector<int64_t> count(nray);
        for (auto &c : count) c = (int64_t)(r.next() % most);
        const std::vector<int64_t> off = prefix(count);
        const size_t per_ray = 24 + (stage ? 8 * (size_t)nvel : 0);
        int64_t at = 0;
        const std::vector<int64_t> bs = batches(off, nvel, stage, per_segment);
        for (int64_t m : bs) {
            const size_t bytes = (size_t)(off[(size_t)(at + m)] - off[(size_t)at]) * per_segment + (size_t)m * per_ray;
            CHECK(bytes <= kSpectraWorkBytes || m == 1);
            over += bytes > kSpectraWorkBytes;
            // and no smaller than it has to be: one more ray would leave the budget, or there is none
            if (at + m < (int64_t)nray)
                CHECK((size_t)(off[(size_t)(at + m + 1)] - off[(size_t)at]) * per_segment + (size_t)(m + 1) * per_ray > kSpectraWorkBytes);
            at += m;
        }
        CHECK(at == (int64_t)nray);
        whole += bs.size() == 1;
        cut += bs.size() > 1;
    }
    CHECK(over > 0 && whole > 20 && cut > 20); // the draws reach all three answers
    std::printf("ray batch rule: ok (%d over the budget, %d whole calls, %d cut)\n", over, whole, cut);
    return 0;
}
