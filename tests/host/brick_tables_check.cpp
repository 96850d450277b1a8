// The host side of the brick sweeps (radiativetransfer_amd/csrc/ftte_bricks.h) against a stub of the HIP runtime (tests/host/stub),
// under the address and undefined-behaviour sanitizers with leak detection: which plan a set of tables holds, when a Sent buffer
// copies, the launch record against a field-by-field fill with literal numbers, the order of a merge's accumulators, the lanes'
// frequency slices, the lanes' streams and events, and what the one-launch forms report after a sweep.
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "ftte_bricks.h"

using namespace ftte;

#define CHECK(cond)                                                                                                \
    do {                                                                                                           \
        if (!(cond)) { std::fprintf(stderr, "ERROR %s:%d: %s\n", __FILE__, __LINE__, #cond); std::exit(1); }       \
    } while (0)

// a plan as the planner leaves it, by hand: 72^3 (ragged: 2 x 9 x 9 bricks), chunk 8, ten tasks, three groups
static BrickPlan hand_plan(long long id)
{
    BrickPlan P;
    P.id = id;
    P.n = 72; P.chunk = 8;
    P.ntu = 2; P.ntv = 9; P.nti = 9; P.up = 128; P.vp = 72;
    P.ut = 16; P.uw = 144; P.nslot = 2;
    P.vface_off = 1000; P.iface_off = 2000; P.uqface_off = 3000; P.face_elems = 5000;
    P.layers.resize(3 * 72);
    for (size_t q = 0; q < P.layers.size(); ++q) P.layers[q].info = (int32_t)(q + 100 * id);
    P.tasks.resize(10);
    for (size_t q = 0; q < P.tasks.size(); ++q) P.tasks[q] = BrickTask{(int16_t)(q % 3), (int16_t)q, (int16_t)id, 0};
    P.groups.resize(3);
    return P;
}

static void check_tables()
{
    const long base = stub().live;
    {
        BrickTables T;
        BrickPlan A = hand_plan(1), B = hand_plan(2), none;
        CHECK(!T.holds(A) && !T.holds(B) && !T.holds(none)); // (a plan nobody has stamped is held by nothing, empty tables included)
        long copies = stub().copies;
        CHECK(T.upload(A) == hipSuccess && T.holds(A) && !T.holds(B));
        CHECK(stub().copies == copies + 2 && stub().live == base + 2); // layers, tasks; no deps, merge blocks or queue in this plan
        CHECK(T.layers[5].info == 105 && T.tasks[9].tu == 9 && T.tasks[9].tv == 1);
        CHECK(T.upload(A) == hipSuccess && stub().copies == copies + 2); // held: nothing is copied
        // another plan into the same tables (the hybrid sweep's after the uniform grid's): A is displaced, and copies again later
        CHECK(T.upload(B) == hipSuccess && T.holds(B) && !T.holds(A) && stub().copies == copies + 4);
        CHECK(T.layers[5].info == 205 && T.tasks[9].tv == 2);
        CHECK(T.upload(A) == hipSuccess && T.holds(A) && !T.holds(B) && stub().copies == copies + 6);
        CHECK(T.layers[5].info == 105 && T.tasks[9].tv == 1 && stub().live == base + 2);
        // a rebuilt plan has another id even where its content is the same
        BrickPlan A2 = hand_plan(1);
        A2.id = 3;
        CHECK(!T.holds(A2));
        // the uniform grid's plan with the one-launch forms' tables and merge blocks
        BrickPlan D = hand_plan(4);
        D.dataflow = D.persistent = true;
        D.deps.assign(10 * kBrickDeps, -1); D.deps[7] = 3;
        D.merge_blocks = {4, 5, 6};
        D.queue = {9, 8, 7, 6};
        copies = stub().copies;
        CHECK(T.upload(D) == hipSuccess && T.holds(D) && stub().copies == copies + 5 && stub().live == base + 5);
        CHECK(T.deps[7] == 3 && T.merge_blocks[2] == 6 && T.queue[0] == 9 && T.queue[3] == 6);

        // a failed allocation: the first one, and one in the middle -- nothing is held, nothing leaks
        BrickTables U;
        stub().fail_next = true;
        CHECK(U.upload(A) != hipSuccess && !U.holds(A) && stub().live == base + 5);
        CHECK(U.layers.reserve(1000) == hipSuccess); // (room for the layers: the next allocation is the tasks')
        stub().fail_next = true;
        CHECK(U.upload(A) != hipSuccess && !U.holds(A) && stub().live == base + 6);
        CHECK(U.upload(A) == hipSuccess && U.holds(A) && stub().live == base + 7);
        // ... and one that displaces a held plan leaves nothing held
        stub().fail_next = true;
        BrickPlan big = hand_plan(5);
        big.tasks.resize(5000);
        CHECK(U.upload(big) != hipSuccess && !U.holds(big) && !U.holds(A));
        CHECK(U.upload(A) == hipSuccess && U.holds(A));
    }
    CHECK(stub().live == base);
}

static void check_sent()
{
    const long base = stub().live;
    {
        Sent<double> S;
        double v[8] = {1, 2, 3, 4, 5, 6, 7, 8};
        long copies = stub().copies;
        CHECK(S.get() == nullptr);
        CHECK(S.send(v, 4) == hipSuccess && stub().copies == copies + 1 && S[3] == 4.0);
        CHECK(S.send(v, 4) == hipSuccess && stub().copies == copies + 1); // identical bytes: one copy
        v[2] = 30;
        CHECK(S.send(v, 4) == hipSuccess && stub().copies == copies + 2 && S[2] == 30.0); // a byte changed: a second copy
        CHECK(S.send(v, 4) == hipSuccess && stub().copies == copies + 2);
        // fewer elements of the same buffer are other bytes
        CHECK(S.send(v, 3) == hipSuccess && stub().copies == copies + 3);
        // the buffer grows: the new one holds nothing
        double *const before = S.get();
        CHECK(S.send(v, 8) == hipSuccess && stub().copies == copies + 4 && S[7] == 8.0 && stub().live == base + 1);
        (void)before;
        CHECK(S.send(v, 8) == hipSuccess && stub().copies == copies + 4);
        // reset: nothing is held, the next send copies
        S.reset();
        CHECK(S.get() == nullptr && stub().live == base);
        CHECK(S.send(v, 8) == hipSuccess && stub().copies == copies + 5 && S[7] == 8.0);
        // a failed allocation: empty, nothing held, and the send after it copies
        double w[16] = {};
        stub().fail_next = true;
        CHECK(S.send(w, 16) != hipSuccess && S.get() == nullptr && stub().live == base && stub().copies == copies + 5);
        CHECK(S.send(v, 8) == hipSuccess && stub().copies == copies + 6);
        // nothing to send: no copy, whatever is held
        CHECK(S.send(v, 0) == hipSuccess && stub().copies == copies + 6);

        // the group records as the sweeps send them: zeroed, filled, compared as bytes
        Sent<BrickGroup> G;
        BrickGroup g[2];
        std::memset(g, 0, sizeof g);
        g[1].org = -1; g[1].ndir = 3;
        copies = stub().copies;
        CHECK(G.send(g, 2) == hipSuccess && G.send(g, 2) == hipSuccess && stub().copies == copies + 1);
        g[1].J = v; // the accumulator moved
        CHECK(G.send(g, 2) == hipSuccess && stub().copies == copies + 2 && G[1].J == v);
    }
    CHECK(stub().live == base);
}

// the parent's field-by-field fill, with this check's numbers written out
static BrickLaunch expected(const BrickGroup *groups, const BrickTask *tasks, const double *uvb, int64_t group_stride, int64_t face_stride, int n, int ntasks,
                            int nnu, int nu0, int chunk, int emit)
{
    static const ftte_consts math = FTTE_CONSTS_INIT;
    BrickLaunch L;
    std::memset(&L, 0, sizeof L);
    L.groups = groups;
    L.tasks = tasks;
    L.uvb = uvb;
    L.group_stride = group_stride;
    L.face_stride = face_stride;
    L.vface_off = 1000; L.iface_off = 2000; L.uqface_off = 3000;
    L.n = n; L.ntasks = ntasks; L.nnu = nnu; L.nu0 = nu0; L.chunk = chunk;
    L.up = 128; L.vp = 72; L.uw = 144; L.ut = 16; L.nslot = 2;
    L.emit = emit;
    L.math = math;
    return L;
}

static void check_launch()
{
    BrickTables T;
    const BrickPlan P = hand_plan(1);
    CHECK(T.upload(P) == hipSuccess);
    BrickGroup g[3];
    std::memset(g, 0, sizeof g);
    CHECK(T.groups.send(g, 3) == hipSuccess);
    double uvb[8] = {};
    // a stage of a lane of the uniform sweep: tasks [3, 7), frequency groups [2, 5), a source function
    BrickLaunch L = brick_launch(P, T, 3, 7, 2, 5, 373248, 5000, uvb, 2);
    BrickLaunch E = expected(T.groups, T.tasks.get() + 3, uvb, 373248, 5000, 72, 4, 3, 2, 8, 2);
    CHECK(!std::memcmp(&L, &E, sizeof L));
    CHECK(L.tiled == 0 && L.ablate == 0 && L.atomic_acc == 0 && L.sub == 0 && L.ticket == nullptr && L.queue == nullptr && L.epoch == 0);
    // the whole task list, every group (the one-launch forms)
    L = brick_launch(P, T, 0, 10, 0, 8, 373248, 5000, uvb, 0);
    E = expected(T.groups, T.tasks, uvb, 373248, 5000, 72, 10, 8, 0, 8, 0);
    CHECK(!std::memcmp(&L, &E, sizeof L));
    // a frequency range alone: the second of three lanes of eight groups
    L = brick_launch(P, T, 0, 10, 2, 5, 373248, 5000, uvb, 0);
    E = expected(T.groups, T.tasks, uvb, 373248, 5000, 72, 10, 3, 2, 8, 0);
    CHECK(!std::memcmp(&L, &E, sizeof L));
    // the hybrid sweep's strides: the base cells between groups, base and fine rings between a direction's groups
    L = brick_launch(P, T, 4, 6, 0, 8, 262144, 7000, uvb, 1);
    E = expected(T.groups, T.tasks.get() + 4, uvb, 262144, 7000, 72, 2, 8, 0, 8, 1);
    CHECK(!std::memcmp(&L, &E, sizeof L));
    // the fine block: its own plan (32^3, chunk 4) and tables; the caller adds `sub`
    BrickTables F;
    BrickPlan Q = hand_plan(2);
    Q.n = 32; Q.chunk = 4;
    CHECK(F.upload(Q) == hipSuccess && F.groups.send(g, 3) == hipSuccess);
    L = brick_launch(Q, F, 1, 2, 0, 8, 32768, 7000, uvb, 0);
    L.sub = 1;
    E = expected(F.groups, F.tasks.get() + 1, uvb, 32768, 7000, 32, 1, 8, 0, 4, 0);
    E.sub = 1;
    CHECK(!std::memcmp(&L, &E, sizeof L) && L.groups != T.groups.get());
}

static void check_lists_and_slices()
{
    DeviceBuffer<double> set[3][kMaxAcc];
    for (int l = 0; l < 3; ++l)
        for (int s = 0; s < 3; ++s) CHECK(set[l][s].reserve(16) == hipSuccess);
    const int nacc[3] = {2, 0, 3}, lane_frame[3] = {0, 0, 2};
    AccList A = acc_list(set, nacc, kOwnFrame);
    CHECK(A.count == 5);
    CHECK(A.acc[0] == set[0][0] && A.acc[1] == set[0][1] && A.acc[2] == set[2][0] && A.acc[3] == set[2][1] && A.acc[4] == set[2][2]);
    CHECK(A.layout[0] == 0 && A.layout[1] == 0 && A.layout[2] == 2 && A.layout[3] == 2 && A.layout[4] == 2);
    A = acc_list(set, nacc, kOwnFrame, 7); // a lane's first element
    CHECK(A.count == 5 && A.acc[0] == set[0][0] + 7 && A.acc[1] == set[0][1] + 7 && A.acc[2] == set[2][0] + 7 && A.acc[4] == set[2][2] + 7);
    A = acc_list(set, nacc, lane_frame, 7); // layout 1 in the frame of layout 0
    CHECK(A.count == 5 && A.acc[2] == set[2][0] + 7 && A.layout[0] == 0 && A.layout[1] == 0 && A.layout[2] == 2 && A.layout[4] == 2);
    const int all[3] = {1, 2, 1};
    A = acc_list(set, all, lane_frame);
    CHECK(A.count == 4 && A.acc[1] == set[1][0] && A.acc[2] == set[1][1] && A.acc[3] == set[2][0]);
    CHECK(A.layout[0] == 0 && A.layout[1] == 0 && A.layout[2] == 0 && A.layout[3] == 2);
    A = acc_list(set, all, kOwnFrame);
    CHECK(A.count == 4 && A.layout[0] == 0 && A.layout[1] == 1 && A.layout[2] == 1 && A.layout[3] == 2);
    const int nothing[3] = {0, 0, 0};
    CHECK(acc_list(set, nothing, kOwnFrame).count == 0);

    const int64_t ncell = 1000;
    for (int nnu = 1; nnu <= 9; ++nnu)
        for (int lanes = 1; lanes <= 4; ++lanes) {
            int next = 0;
            for (int lane = 0; lane < lanes; ++lane) {
                const LaneSlice S = lane_slice(nnu, lane, lanes, ncell);
                CHECK(S.nu0 == next && S.nu0 == nnu * lane / lanes && S.nu1 == nnu * (lane + 1) / lanes && S.nu1 >= S.nu0);
                CHECK(S.first == (size_t)S.nu0 * 1000 && S.bytes == 8u * (size_t)(S.nu1 - S.nu0) * 1000);
                next = S.nu1;
            }
            CHECK(next == nnu);
        }
    CHECK(lane_slice(3, 1, 2, 1ll << 32).first == (size_t)1 << 32); // (64-bit: a group of 2^32 cells)
}

static void check_lanes_and_dataflow()
{
    const long base = stub().live;
    {
        std::vector<Stream> streams;
        std::vector<Event> done, points;
        CHECK(ensure_lanes(streams, done, 0) == hipSuccess && streams.empty() && done.empty() && stub().live == base);
        CHECK(ensure_lanes(streams, done, 2) == hipSuccess && streams.size() == 2 && done.size() == 2 && stub().live == base + 4);
        CHECK(ensure_lanes(streams, done, 1) == hipSuccess && streams.size() == 2 && stub().live == base + 4);
        CHECK(ensure_events(points, 5, hipEventDisableTiming) == hipSuccess && points.size() == 5 && points[4].get() && stub().live == base + 9);
        stub().fail_next = true;
        CHECK(ensure_events(points, 7, hipEventDisableTiming) != hipSuccess && points.size() == 5 && stub().live == base + 9);
        stub().fail_next = true;
        CHECK(ensure_lanes(streams, done, 3) != hipSuccess && streams.size() == 2 && done.size() == 2);

        BrickTables T;
        BrickPlan P = hand_plan(1);
        P.dataflow = true;
        P.deps.assign(10 * kBrickDeps, -1);
        CHECK(T.upload(P) == hipSuccess);
        BrickDataflow F;
        BrickLaunch L;
        std::memset(&L, 0, sizeof L);
        CHECK(F.check_after_sweep(P.qload) == nullptr); // (no such sweep yet)
        CHECK(F.prepare(L, T, 80, nullptr) == hipSuccess);
        CHECK(L.epoch == 1 && L.done == F.done.get() && L.ticket == F.sync.get() && L.error == F.sync.get() + 32 * kBrickQueues && L.deps == T.deps.get());
        CHECK(F.done[79] == 0 && F.sync[32 * kBrickQueues] == 0 && F.error[0] == 0);
        F.done[3] = 1; // (a brick finished)
        CHECK(F.prepare(L, T, 80, nullptr) == hipSuccess && L.epoch == 2 && F.done[3] == 1); // the flags stay between the epochs
        F.epoch = 0xffffffffu;
        CHECK(F.prepare(L, T, 80, nullptr) == hipSuccess && L.epoch == 1 && F.done[3] == 0); // ... and are zeroed when the epoch wraps
        CHECK(F.prepare(L, T, 800, nullptr) == hipSuccess && L.epoch == 1 && F.done[799] == 0); // ... and when they are reallocated
        CHECK(F.read_back(P, nullptr) == hipSuccess && F.check_after_sweep(P.qload) == nullptr);
        F.sync[32 * kBrickQueues] = 1; // a brick gave up
        CHECK(F.read_back(P, nullptr) == hipSuccess);
        const char *why = F.check_after_sweep(P.qload);
        CHECK(why && std::strstr(why, "gave up") && F.check_after_sweep(P.qload) == nullptr);
        // the persistent form: every queue's ticket must have reached the queue's length
        P.persistent = true;
        P.qlen[0] = 5; P.qlen[1] = 5;
        CHECK(F.prepare(L, T, 800, nullptr) == hipSuccess);
        F.sync[0] = 5; F.sync[32] = 5;
        CHECK(F.read_back(P, nullptr) == hipSuccess && F.check_after_sweep(P.qload) == nullptr);
        CHECK(F.prepare(L, T, 800, nullptr) == hipSuccess);
        F.sync[0] = 7; F.sync[32] = 4; // (workgroups that found queue 0 empty drew tickets as well)
        CHECK(F.read_back(P, nullptr) == hipSuccess);
        why = F.check_after_sweep(P.qload);
        CHECK(why && std::strstr(why, "undrained") && F.check_after_sweep(P.qload) == nullptr);
    }
    CHECK(stub().live == base);
}

int main()
{
    check_tables();
    check_sent();
    check_launch();
    check_lists_and_slices();
    check_lanes_and_dataflow();
    CHECK(stub().live == 0 && !stub().fail_next);
    std::printf("brick tables under the sanitizers: ok\n");
    return 0;
}
