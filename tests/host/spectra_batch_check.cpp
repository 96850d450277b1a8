// ftte::spectra_batch_lines (radiativetransfer_amd/csrc/ftte_spectra.h) against a stub of the HIP runtime (tests/host/stub), as a
// program of its own, with and without the sanitizers (tests/test_spectra_host.py): the rule that keeps what a batch of sightlines
// stages -- three doubles of summaries per line, nvel doubles of tau where tau is staged, most_segments records where a line exceeds
// a chunk -- under kSpectraWorkBytes.  Known values written out, the property over random arguments, and with a file of
// "nlines nvel stage_tau most_segments" rows the function's answers one per row, for the tests' restatement of the rule
// (tests/_spectra.py: batch_lines) to be held against.
#include <cstdint>
#include <cstdio>
#include <cstdlib>

#include "ftte_spectra.h"

using namespace ftte;

#define CHECK(cond)                                                                                                \
    do {                                                                                                           \
        if (!(cond)) { std::fprintf(stderr, "ERROR %s:%d: %s\n", __FILE__, __LINE__, #cond); std::exit(1); }       \
    } while (0)

// what the tests' restatement takes as given
static_assert(kSpectraWorkBytes == (size_t)1 << 26, "the budget of a batch");
static_assert(kSpectraChunk == 512 && kSpectraLanes == 256 && kSpectraPassPixels == 1024, "chunk, lanes, pass");
static_assert(sizeof(ftte_spectra_seg) == 32, "a record");

struct Lcg {
    uint64_t s;
    uint64_t next() { s = s * 6364136223846793005ull + 1442695040888963407ull; return s >> 11; }
};

static size_t per_line(int64_t nvel, bool stage_tau, int64_t most)
{
    return 24 + (stage_tau ? 8 * (size_t)nvel : 0) + (most > 512 ? 32 * (size_t)most : 0);
}

int main(int argc, char **argv)
{
    if (argc > 1) {
        std::FILE *f = std::fopen(argv[1], "r");
        if (!f) { std::printf("cannot read %s\n", argv[1]); return 2; }
        long long nlines, nvel, most;
        int stage;
        while (std::fscanf(f, "%lld %lld %d %lld", &nlines, &nvel, &stage, &most) == 4)
            std::printf("%lld\n", (long long)spectra_batch_lines(nlines, nvel, stage != 0, most));
        std::fclose(f);
        return 0;
    }
    CHECK(spectra_batch_lines(4096, 70, false, 1027) == 2040);
    CHECK(spectra_batch_lines(4096, 70, true, 1027) == 2006);
    CHECK(spectra_batch_lines(65536, 1024, true, 512) == 8168); // most == kSpectraChunk adds no spill term
    CHECK(spectra_batch_lines(65536, 1024, true, 513) < 8168);
    CHECK(spectra_batch_lines(100, 1024, true, 4) == 100);
    CHECK(spectra_batch_lines(5, 1 << 24, true, 4) == 1); // one line over the budget still gets a batch
    CHECK(spectra_batch_lines(0, 1024, true, 4) == 1);
    CHECK(spectra_batch_lines(0, 0, false, 0) == 1);
    CHECK(spectra_batch_lines(-3, 70, true, 1027) == 1);
    CHECK(spectra_batch_lines(4608, 4096, true, 4) == 2046);
    CHECK(spectra_batch_lines(1280, 16384, true, 4) == 511);

    Lcg r{20261021ull};
    int over = 0, whole = 0, cut = 0;
    for (int q = 0; q < 600; ++q) {
        const int64_t nlines = (int64_t)(r.next() % (q % 3 ? 100000 : 40)), nvel = (int64_t)(r.next() % (q % 5 ? 40000 : (1 << 25)));
        const bool stage = r.next() & 1;
        const int64_t most = (int64_t)(r.next() % (q % 7 ? 3000 : 4000000));
        const int64_t batch = spectra_batch_lines(nlines, nvel, stage, most);
        CHECK(batch >= 1 && batch <= (nlines > 1 ? nlines : 1));
        const size_t bytes = (size_t)batch * per_line(nvel, stage, most);
        CHECK(bytes <= kSpectraWorkBytes || batch == 1);
        // and no smaller than it has to be: one more line would leave the budget, or there is none
        CHECK(batch == nlines || nlines < 1 || (size_t)(batch + 1) * per_line(nvel, stage, most) > kSpectraWorkBytes);
        over += bytes > kSpectraWorkBytes;
        whole += batch == nlines;
        cut += batch > 1 && batch < nlines;
    }
    CHECK(over > 0 && whole > 50 && cut > 50); // the draws reach all three answers
    std::printf("spectra batch rule: ok (%d over the budget, %d whole maps, %d cut)\n", over, whole, cut);
    return 0;
}
