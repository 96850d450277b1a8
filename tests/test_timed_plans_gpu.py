"""The plans the benchmark times, against the oracle.

bench.py's default run (256^3 cells x 8 frequency groups x 96 directions) takes a brick plan in which direction groups share
J accumulators: above 64 cells a side, where every brick count is even, izones of opposite brick-stage parity are paired on one
accumulator and the later group reads, adds and stores without atomics (csrc/ftte_planner.cpp, plan_brick_groups).  Determinism
and linearity cannot see a contribution that is lost the same way on every run; these tests compare J with the oracle (device
arithmetic, ARITH_DEVICE) to the rounding of the sum over directions, per cell, with no absolute slack:
  * the headline run end to end: what bench.py itself timed and dumped;
  * 128^3 -- aligned, every brick count even -- under every option that reshapes the plan or the launch, each proving through
    the library's counters which path ran (the one-launch forms fall back without notice);
  * the shapes the ranks of a 2-, 4-, 8- and 16-rank run of 192 directions execute (radiativetransfer_amd.distributed.Shard2D).
"""
import json
import os
import subprocess
import sys
import time

import numpy as np
import pytest

import _oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402

pytestmark = pytest.mark.gpu

SUM_RTOL = 64 * np.finfo(np.float64).eps
CHECKED_GROUPS = [0, 7]   # of the rank shapes: the thickest group and the thinnest (the attenuation pair's thin-range polynomial)


def _close(J, ref, what):
    rel = np.abs(J - ref) / np.abs(ref)
    bad = ~(np.abs(J - ref) <= SUM_RTOL * np.abs(ref))
    assert not bad.any(), f"{what}: {int(bad.sum())} cells beyond {SUM_RTOL:.1e} relative, worst {np.nanmax(rel):.3e}"


def test_the_headline_run_against_the_oracle(tmp_path):
    """bench.py --steps 2 --warmup 1 with every default (256^3 x 8 groups x 96 directions, the library's default options): the
    J of its last timed step -- the seeded sample of cells bench.dump_outputs writes -- equals the oracle's to SUM_RTOL in
    every sampled cell of all eight groups (the oracle runs on the host while bench.py runs on the GPU: about 30 s on 16
    threads).  The plan is the one the verdict describes: a second context on the same grid and directions reports 36
    direction groups on 8 accumulators, so the passes of an izone and izone pairs really share (observed on the MI355X; the
    assertion is only that sharing happened)."""
    import radiativetransfer_amd as rt
    from radiativetransfer_amd import synthetic
    n, nnu, ndir = 256, 8, 96
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1",
           "--dump-outputs", str(tmp_path / "out")]
    t0 = time.perf_counter()
    run = subprocess.Popen(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, cwd=ROOT)
    try:
        # the oracle on the host while the benchmark runs on the GPU
        kappa, uvb, box = synthetic.uniform_workload(n, nnu, seed=12345, tau_median=0.1)
        phi, theta, w = bench.directions(ndir)
        ref = O.sweep_uniform_parallel(n, kappa, box, phi, theta, w, uvb, arith=O.ARITH_DEVICE)
        t_oracle = time.perf_counter() - t0
        out, err = run.communicate(timeout=600)
    finally:
        if run.poll() is None:
            run.kill()
            run.communicate()
    assert run.returncode == 0, err[-3000:]
    line = json.loads([ln for ln in out.splitlines() if ln.startswith("{")][-1])
    assert line["steps"] == 2 and line["warmup"] == 1 and line["ms_per_step"] > 0
    J = np.load(tmp_path / "out" / "J.npy")
    # bench's own sampling rule, applied to the cell index of every column
    bench.dump_outputs(tmp_path / "index", {"J": np.broadcast_to(np.arange(n ** 3, dtype=np.float64), (nnu, n ** 3))})
    idx = np.load(tmp_path / "index" / "J.npy")[0].astype(np.int64)
    assert J.shape == (nnu, idx.size) and idx.size < n ** 3 and np.all(np.diff(idx) > 0)
    assert np.all(J > 0) and np.all(np.isfinite(J))
    for nu in range(nnu):
        _close(J[nu], ref[nu, idx], f"group {nu}")
    print(f"headline: oracle {t_oracle:.1f} s on {O.oracle_threads()} threads, {idx.size} cells x {nnu} groups checked")
    del ref
    # the plan bench's context ran: same grid, groups and directions in a context of this process
    with rt.DiffuseTransfer() as eng:
        eng.set_uniform_grid(n, box)
        eng.set_opacity(kappa)
        eng.transport(phi, theta, w, uvb)
        groups, accs = eng.counter("brick_groups"), eng.counter("brick_accumulators")
        form, dataflow = eng.counter("brick_form"), eng.counter("brick_dataflow")
    print(f"headline plan: {groups} direction groups on {accs} accumulators, brick form {form}, dataflow {dataflow}")
    assert 0 < accs < groups and form == 0 and dataflow == 0


# ---- 128^3: every option that reshapes the plan or the launch --------------------------------------------------------------

N_ALIGNED = 128


@pytest.fixture(scope="module")
def aligned():
    from radiativetransfer_amd import synthetic
    n, nnu = N_ALIGNED, 8
    kappa, uvb, box = synthetic.uniform_workload(n, nnu, seed=12345, tau_median=0.1)
    phi, theta, w = bench.directions(96)
    ref = O.sweep_uniform_parallel(n, kappa, box, phi, theta, w, uvb, arith=O.ARITH_DEVICE)
    return dict(n=n, nnu=nnu, kappa=kappa, uvb=uvb, box=box, phi=phi, theta=theta, w=w, ref=ref)


@pytest.fixture()
def aligned_engine(aligned):
    import radiativetransfer_amd as rt
    with rt.DiffuseTransfer() as eng:
        eng.set_uniform_grid(aligned["n"], aligned["box"])
        eng.set_opacity(aligned["kappa"])
        yield eng


def _sweep(eng, a, **opts):
    for k, v in opts.items():
        eng.set_option(k, v)
    return eng.transport(a["phi"], a["theta"], a["w"], a["uvb"])


def _path(eng):
    return {k: eng.counter(k) for k in ("brick_form", "brick_dataflow", "brick_groups", "brick_accumulators", "brick_chunk",
                                        "brick_queue_mix")}


def test_aligned_default_plan_shares_and_repeats_bit_for_bit(aligned, aligned_engine):
    a = aligned
    J = _sweep(aligned_engine, a)
    p = _path(aligned_engine)
    assert p["brick_form"] == 0 and p["brick_dataflow"] == 0 and 0 < p["brick_accumulators"] < p["brick_groups"], p
    _close(J, a["ref"], f"default {p}")
    assert np.array_equal(J, _sweep(aligned_engine, a))


def test_aligned_accumulator_sharing(aligned, aligned_engine):
    """share 0: an accumulator per direction group; 1: the passes of one izone share; 2: izone pairs of opposite parity too."""
    a = aligned
    accs = {}
    for share in (0, 1, 2):
        J = _sweep(aligned_engine, a, share=share)
        p = _path(aligned_engine)
        accs[share] = p["brick_accumulators"]
        assert p["brick_form"] == 0 and p["brick_dataflow"] == 0, p
        if share == 0:
            assert p["brick_accumulators"] == p["brick_groups"], p
        _close(J, a["ref"], f"share {share} {p}")
    assert accs[2] < accs[1] < accs[0], accs


@pytest.mark.parametrize("team", [0, 2])
def test_aligned_brick_forms(aligned, aligned_engine, team):
    a = aligned
    J = _sweep(aligned_engine, a, team=team)
    p = _path(aligned_engine)
    assert p["brick_form"] == team and p["brick_dataflow"] == 0 and p["brick_accumulators"] < p["brick_groups"], p
    _close(J, a["ref"], f"team {team} {p}")


@pytest.mark.parametrize("lanes", [1, 4])
def test_aligned_streams(aligned, aligned_engine, lanes):
    a = aligned
    J = _sweep(aligned_engine, a, lanes=lanes)
    p = _path(aligned_engine)
    assert p["brick_form"] == 0 and p["brick_dataflow"] == 0 and p["brick_accumulators"] < p["brick_groups"], p
    _close(J, a["ref"], f"lanes {lanes} {p}")


@pytest.mark.parametrize("chunk", [8, 32])
def test_aligned_brick_lengths(aligned, aligned_engine, chunk):
    a = aligned
    J = _sweep(aligned_engine, a, chunk=chunk)
    p = _path(aligned_engine)
    assert p["brick_chunk"] == chunk and p["brick_form"] == 0 and p["brick_dataflow"] == 0, p
    assert p["brick_accumulators"] < p["brick_groups"], p
    _close(J, a["ref"], f"chunk {chunk} {p}")


@pytest.mark.parametrize("dataflow", [1, 2, 3])
def test_aligned_one_launch_forms(aligned, aligned_engine, dataflow):
    """One launch whose bricks wait on flags (1; 2 with write-through stores) and persistent workgroups fed by a queue per XCD
    (3): brick_dataflow shows the form that ran -- the option falls back to 1 without the XCD census and to 0 off alignment."""
    a = aligned
    J = _sweep(aligned_engine, a, dataflow=dataflow)
    p = _path(aligned_engine)
    assert p["brick_dataflow"] == dataflow and p["brick_form"] == 0 and p["brick_accumulators"] < p["brick_groups"], p
    _close(J, a["ref"], f"dataflow {dataflow} {p}")


@pytest.mark.parametrize("queue_mix", [0, 1, 2])
def test_aligned_persistent_queue_layouts(aligned, aligned_engine, queue_mix):
    a = aligned
    J = _sweep(aligned_engine, a, dataflow=3, queue_mix=queue_mix)
    p = _path(aligned_engine)
    assert p["brick_dataflow"] == 3 and p["brick_queue_mix"] == queue_mix and p["brick_form"] == 0, p
    _close(J, a["ref"], f"queue_mix {queue_mix} {p}")


# ---- what the ranks of a sharded 192-direction run execute, at 128^3 --------------------------------------------------------

@pytest.fixture(scope="module")
def halves(aligned):
    """The oracle for groups 0 and 7 over each half of the 192 directions of nside 4 (weights 1/192), once."""
    a = aligned
    phi, theta, w = bench.directions(192)
    out = {}
    for h in (0, 1):
        s = slice(96 * h, 96 * (h + 1))
        ref = O.sweep_uniform_parallel(a["n"], a["kappa"][CHECKED_GROUPS], a["box"], phi[s], theta[s], w[s], a["uvb"][CHECKED_GROUPS],
                                       arith=O.ARITH_DEVICE)
        for row, nu in enumerate(CHECKED_GROUPS):
            out[nu, h] = ref[row]
    return dict(phi=phi, theta=theta, w=w, ref=out)


@pytest.mark.parametrize("world", [2, 4, 8, 16])
def test_rank_shapes_of_a_sharded_run(aligned, halves, world):
    """Shard2D(rank, world, 8): each rank sweeps its frequency groups over its slice of the 192 directions.  The ranks that hold
    group 0 or group 7 run their whole shape; those two groups are compared with the oracle over the same directions.  A rank
    with a single group takes the pair form (brick_form 2)."""
    import radiativetransfer_amd as rt
    from radiativetransfer_amd.distributed import Shard2D
    a, hv = aligned, halves
    seen = set()
    for rank in range(world):
        sh = Shard2D(rank, world, a["nnu"])
        lo, hi = sh.groups
        mine = [nu for nu in CHECKED_GROUPS if lo <= nu < hi]
        if not mine:
            continue
        phi, theta, w = sh.directions(hv["phi"], hv["theta"], hv["w"])
        first = int(np.flatnonzero(hv["phi"] == phi[0])[0])
        assert np.array_equal(phi, hv["phi"][first:first + len(phi)]) and len(phi) in (96, 192) and first in (0, 96)
        with rt.DiffuseTransfer() as eng:
            eng.set_uniform_grid(a["n"], a["box"])
            eng.set_opacity(a["kappa"][lo:hi])
            J = eng.transport(phi, theta, w, a["uvb"][lo:hi])
            form = eng.counter("brick_form")
        if hi - lo == 1:
            assert form == 2, (world, rank, form)
        for nu in mine:
            ref = hv["ref"][nu, first // 96] if len(phi) == 96 else hv["ref"][nu, 0] + hv["ref"][nu, 1]
            _close(J[nu - lo], ref, f"world {world} rank {rank} groups {lo}..{hi - 1} group {nu}")
            seen.add(nu)
    assert seen == set(CHECKED_GROUPS)
