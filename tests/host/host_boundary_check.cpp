// HostBoundary (radiativetransfer_amd/csrc/ftte_host.h) against a stub of the HIP runtime (tests/host/stub), under the address and
// undefined-behaviour sanitizers with leak detection.  The stub runs the laziest legal schedule: a copy is carried out when the
// host waits for it, so host code that rewrites a staging block before the transfer out of it, or reads one before the transfer
// into it, delivers wrong bytes here every time.  Blocks of 4096 bytes.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "ftte_host.h"

using namespace ftte;

#define CHECK(cond)                                                                                                \
    do {                                                                                                           \
        if (!(cond)) { std::fprintf(stderr, "ERROR %s:%d: %s\n", __FILE__, __LINE__, #cond); std::exit(1); }       \
    } while (0)

constexpr size_t kBlock = 4096, kGuard = 64;
const size_t kSizes[] = {1, 4095, 4096, 4097, 8192, 8193, 5 * 4096 + 17};
constexpr unsigned char kUntouched = 0xA5;

using Bytes = std::vector<unsigned char>;

// `bytes` of a seeded pattern (xorshift64*)
static Bytes pattern(size_t bytes, uint64_t seed)
{
    Bytes v(bytes);
    uint64_t x = seed * 0x9E3779B97F4A7C15ull + 1;
    for (auto &b : v) { x ^= x >> 12; x ^= x << 25; x ^= x >> 27; b = (unsigned char)((x * 0x2545F4914F6CDD1Dull) >> 56); }
    return v;
}
static Bytes target(size_t bytes) { return Bytes(bytes + kGuard, kUntouched); }
// the first src.size() bytes are src's, the guard behind them is untouched
static bool holds(const Bytes &dst, const Bytes &src)
{
    for (size_t q = 0; q < src.size(); ++q)
        if (dst[q] != src[q]) return false;
    for (size_t q = src.size(); q < dst.size(); ++q)
        if (dst[q] != kUntouched) return false;
    return dst.size() == src.size() + kGuard;
}
static void overwrite(Bytes &v) { for (auto &b : v) b = (unsigned char)~b; }

struct Streams {
    Stream a, b;
    Streams() { CHECK(a.create() == hipSuccess && b.create() == hipSuccess); }
    void wait() { CHECK(hipStreamSynchronize(a) == hipSuccess && hipStreamSynchronize(b) == hipSuccess); }
};

// Both loops deliver exact bytes and touch nothing beyond the size asked for
static void check_exact_bytes()
{
    Streams S;
    HostBoundary H(kBlock);
    uint64_t seed = 1;
    for (const size_t bytes : kSizes) {
        // to the device: back before it has arrived, the caller's array is the caller's again
        Bytes src = pattern(bytes, seed++), dev = target(bytes);
        const Bytes sent = src;
        CHECK(H.send(S.a, dev.data(), src.data(), bytes) == hipSuccess);
        overwrite(src);
        CHECK(H.outstanding(0) && H.outstanding(1) == (bytes > kBlock));
        S.wait();
        CHECK(holds(dev, sent));
        // to the host (other bytes than the blocks still hold): in the caller's array on return, the blocks it used waited for
        const Bytes on_device = pattern(bytes, 100 + seed);
        Bytes back = target(bytes);
        CHECK(H.fetch(S.a, back.data(), on_device.data(), bytes) == hipSuccess);
        CHECK(holds(back, on_device));
        CHECK(!H.outstanding(0) && !H.outstanding(1));
        S.wait();
    }
    // nothing to move: nothing moves, nothing is left outstanding
    Bytes none = target(0);
    CHECK(H.send(S.a, none.data(), none.data(), 0) == hipSuccess && H.fetch(S.a, none.data(), none.data(), 0) == hipSuccess);
    CHECK(holds(none, Bytes()) && !H.outstanding(0) && !H.outstanding(1));
}

// Two lanes: a send on one stream, then one on another with no wait in between.  The second must not overwrite a block the first
// still has outstanding.
static void check_two_lanes()
{
    for (const size_t first : kSizes)
        for (const size_t second : kSizes) {
            Streams S;
            HostBoundary H(kBlock);
            Bytes s1 = pattern(first, 11), s2 = pattern(second, 12), d1 = target(first), d2 = target(second);
            const Bytes sent1 = s1, sent2 = s2;
            CHECK(H.send(S.a, d1.data(), s1.data(), first) == hipSuccess);
            // (as brick_sweep orders the lanes' opacities on the link)
            Event up;
            CHECK(up.create(hipEventDisableTiming) == hipSuccess && hipEventRecord(up, S.a) == hipSuccess);
            CHECK(hipStreamWaitEvent(S.b, up, 0) == hipSuccess);
            CHECK(H.send(S.b, d2.data(), s2.data(), second) == hipSuccess);
            overwrite(s1); overwrite(s2);
            CHECK(hipStreamSynchronize(S.b) == hipSuccess); // (what its hipStreamWaitEvent stood for is carried out with it)
            CHECK(holds(d1, sent1) && holds(d2, sent2));
            // the first lane's J comes back through the blocks both lanes have used
            Bytes back = target(first);
            CHECK(H.fetch(S.a, back.data(), d1.data(), first) == hipSuccess);
            CHECK(holds(back, sent1));
            S.wait();
            CHECK(holds(d1, sent1) && holds(d2, sent2));
        }
}

// A sequence that did not come to its end: a send whose stream nobody waits for (brick_sweep returning an error behind a lane's
// upload), then a send or a fetch on another stream.  The first one's bytes still arrive exactly.  (The upload() of before this
// owner started from "no block is busy" and would have filled block 0 anew under the first transfer.)
static void check_abandoned_send(bool then_fetch)
{
    for (const size_t first : kSizes)
        for (const size_t second : kSizes) {
            Streams S;
            HostBoundary H(kBlock);
            Bytes s1 = pattern(first, 21), d1 = target(first);
            const Bytes sent1 = s1;
            CHECK(H.send(S.a, d1.data(), s1.data(), first) == hipSuccess);
            overwrite(s1);
            const Bytes sent2 = pattern(second, 22);
            Bytes s2 = sent2, d2 = target(second), back = target(second);
            if (then_fetch) {
                CHECK(H.fetch(S.b, back.data(), sent2.data(), second) == hipSuccess);
                CHECK(holds(back, sent2));
                // whoever waited has cleared the flag, and only that one: the fetch waited for the blocks it used
                CHECK(!H.outstanding(0) && H.outstanding(1) == (first > kBlock && second <= kBlock));
            } else {
                CHECK(H.send(S.b, d2.data(), s2.data(), second) == hipSuccess);
                overwrite(s2);
                CHECK(hipStreamSynchronize(S.b) == hipSuccess);
                CHECK(holds(d2, sent2));
                CHECK(H.outstanding(0) && H.outstanding(1) == (first > kBlock || second > kBlock));
            }
            S.wait(); // only now is the first stream waited for as a whole
            CHECK(holds(d1, sent1));
        }
}

// A fetch directly after a send, on the same stream and on another: the blocks change hands correctly
static void check_fetch_after_send()
{
    for (const size_t up : kSizes)
        for (const size_t down : kSizes)
            for (int other = 0; other < 2; ++other) {
                Streams S;
                HostBoundary H(kBlock);
                const Bytes sent = pattern(up, 31), on_device = pattern(down, 32);
                Bytes src = sent, dev = target(up), back = target(down);
                CHECK(H.send(S.a, dev.data(), src.data(), up) == hipSuccess);
                CHECK(H.fetch(other ? S.b : S.a, back.data(), on_device.data(), down) == hipSuccess);
                CHECK(holds(back, on_device));
                CHECK(!H.outstanding(0));
                // and a send behind the fetch finds the blocks free or waits for them
                Bytes again = target(up);
                CHECK(H.send(S.b, again.data(), src.data(), up) == hipSuccess);
                S.wait();
                CHECK(holds(dev, sent) && holds(again, sent));
            }
}

static void check_ranges()
{
    std::vector<char> mem(4096);
    char *const m = mem.data();
    std::vector<char> theirs(256);
    char *const t = theirs.data();
    const long pins = stub().pin_calls;
    {
        HostBoundary H(kBlock);
        CHECK(!H.contains(m, 1) && H.unpin(m) == hipErrorHostMemoryNotRegistered);
        // two ranges with a gap: [100, 200) and [300, 400)
        CHECK(H.pin(m + 100, 100) == hipSuccess && H.pin(m + 300, 100) == hipSuccess);
        CHECK(stub().pinned.size() == 2 && stub().pin_calls == pins + 2);
        CHECK(H.contains(m + 100, 100) && H.contains(m + 100, 1) && H.contains(m + 199, 1) && H.contains(m + 150, 50));
        CHECK(!H.contains(m + 99, 1) && !H.contains(m + 99, 2) && !H.contains(m + 200, 1) && !H.contains(m + 199, 2) && !H.contains(m + 100, 101));
        CHECK(H.contains(m + 300, 100) && !H.contains(m + 299, 2) && !H.contains(m + 399, 2));
        CHECK(!H.contains(m + 100, 300) && !H.contains(m + 199, 102)); // across the gap
        // a contained range: no call of the runtime, no second range
        CHECK(H.pin(m + 100, 100) == hipSuccess && H.pin(m + 120, 30) == hipSuccess);
        CHECK(stub().pin_calls == pins + 2 && stub().pinned.size() == 2 && H.pinned(m + 100) && !H.pinned(m + 120));
        // a failed pin leaves no range
        stub().fail_pin_next = true;
        CHECK(H.pin(m + 500, 100) == hipErrorOutOfMemory);
        CHECK(!H.contains(m + 500, 1) && H.unpin(m + 500) == hipErrorHostMemoryNotRegistered && stub().pinned.size() == 2);
        CHECK(H.pin(m + 500, 100) == hipSuccess && H.contains(m + 500, 100) && stub().pinned.size() == 3);
        // unpinning: an unknown base (inside a range is not its base) is reported and changes nothing
        CHECK(H.unpin(m + 120) == hipErrorHostMemoryNotRegistered && H.unpin(m) == hipErrorHostMemoryNotRegistered);
        CHECK(stub().pinned.size() == 3 && H.contains(m + 120, 30));
        CHECK(H.unpin(m + 500) == hipSuccess && !H.contains(m + 500, 1) && stub().pinned.size() == 2);
        CHECK(H.unpin(m + 500) == hipErrorHostMemoryNotRegistered);

        // what a sibling context pinned: learnt, never pinned or unpinned here
        CHECK(hipHostRegister(t, 256, hipHostRegisterPortable) == hipSuccess);
        const long calls = stub().pin_calls;
        H.learn(t, 256);
        H.learn(t, 256); // a second ftte_host_register of the same array on a multi-device context
        CHECK(H.contains(t, 256) && H.contains(t + 255, 1) && !H.contains(t, 257) && !H.pinned(t));
        CHECK(H.pin(t + 16, 16) == hipSuccess && stub().pin_calls == calls); // contained: as for the own ones
        CHECK(H.unpin(t) == hipErrorHostMemoryNotRegistered && H.contains(t, 256));
        H.forget(t);
        CHECK(!H.contains(t, 1) && !H.contains(t + 16, 16)); // learnt twice, forgotten once: nothing is left
        H.forget(t);
        H.learn(t, 100);
        H.learn(t, 200); // not contained: a second range with the same base; one forget takes both
        H.forget(t);
        CHECK(!H.contains(t, 1));
        H.forget(m + 100); // not a learnt one: stays
        CHECK(H.contains(m + 100, 100));
        H.learn(t, 256);
        CHECK(stub().pinned.size() == 3 && stub().pinned.count(t) == 1);
    } // the owner goes with two ranges of its own and a learnt one
    CHECK(stub().pinned.size() == 1 && stub().pinned.count(t) == 1); // exactly its own are unpinned: the sibling's stays
    CHECK(hipHostUnregister(t) == hipSuccess && stub().pinned.empty());
}

// A block or an event that cannot be had (a block is asked for when its first piece comes): the error comes back, the next call
// asks again for what is missing, nothing leaks
static void check_failed_allocation()
{
    const long base = stub().live;
    {
        Streams S;
        const Bytes sent = pattern(3 * kBlock + 5, 41);
        for (int k = 1; k <= 4; ++k) { // the first block, its event, the second block, its event
            HostBoundary H(kBlock);
            Bytes src = sent, dev = target(sent.size()), back = target(sent.size());
            stub().fail_countdown = k;
            CHECK(H.send(S.a, dev.data(), src.data(), src.size()) == hipErrorOutOfMemory);
            CHECK(stub().live == base + 2 + (k - 1) && H.outstanding(0) == (k > 2) && !H.outstanding(1));
            stub().fail_countdown = 1;
            CHECK(H.fetch(S.b, back.data(), sent.data(), sent.size()) == hipErrorOutOfMemory);
            CHECK(stub().live == base + 2 + (k - 1) && holds(back, Bytes(sent.size(), kUntouched)));
            CHECK(H.send(S.a, dev.data(), src.data(), src.size()) == hipSuccess);
            CHECK(stub().live == base + 2 + 4);
            CHECK(H.fetch(S.b, back.data(), sent.data(), sent.size()) == hipSuccess);
            CHECK(stub().live == base + 2 + 4 && holds(back, sent));
            S.wait();
            CHECK(holds(dev, sent));
            CHECK(H.J_dev.reserve(10) == hipSuccess && stub().live == base + 2 + 5);
        }
        CHECK(stub().live == base + 2);
        // an array within one block never asks for the second
        HostBoundary H(kBlock);
        Bytes src = pattern(kBlock, 42), dev = target(kBlock);
        CHECK(H.send(S.a, dev.data(), src.data(), kBlock) == hipSuccess && stub().live == base + 2 + 2);
        S.wait();
        CHECK(holds(dev, src));
    }
    CHECK(stub().live == base && g_device_objects.load() == base);
}

int main()
{
    CHECK(stub().live == 0);
    for (int lazy = 1; lazy >= 0; --lazy) { // and with streams that run everything at once, as every other host check has them
        stub().lazy = lazy != 0;
        check_exact_bytes();
        check_two_lanes();
        check_abandoned_send(false);
        check_abandoned_send(true);
        check_fetch_after_send();
        check_failed_allocation();
    }
    check_ranges();
    CHECK(stub().live == 0 && g_device_objects.load() == 0);
    std::printf("host boundary under the sanitizers: ok\n");
    return 0;
}
