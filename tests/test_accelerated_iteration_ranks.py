"""The accelerated source iteration over ranks (tools/bench_config5.py --accelerate=... under torch.distributed.run), rehearsed on
one GPU: the ranks share GPU 0 and the collectives run on host copies over gloo.  Two ranks split the eight frequency groups: a
rank computes the diagonal of its groups, nothing is summed, Ng's dot products are local to the rank that holds the group -- so
every group's J and the printed history equal the single-process run's bit for bit."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("scheme", ["diagonal", "diagonal+ng"])
def test_accelerated_iteration_over_two_ranks_rehearsed_on_one_gpu(tmp_path, scheme):
    from radiativetransfer_amd.distributed import Shard2D
    script = os.path.join(ROOT, "tools", "bench_config5.py")
    one, many = tmp_path / "one", tmp_path / "many"
    one.mkdir(); many.mkdir()
    steps, ranks = "9", 2   # (Ng extrapolates after steps 4 and 8)
    run = subprocess.run([sys.executable, script, "64", steps, f"--accelerate={scheme}", f"--dump={one}"], capture_output=True, text=True,
                         timeout=600, cwd=ROOT)
    assert run.returncode == 0, run.stderr[-3000:]
    port = 37600 + os.getpid() % 2000 + len(scheme)
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={ranks}", "--master-addr", "127.0.0.1",
           "--master-port", str(port), script, "64", steps, "--rehearse-on-one-gpu", f"--accelerate={scheme}", f"--dump={many}"]
    multi = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert multi.returncode == 0, multi.stderr[-3000:]
    history = lambda out: [ln.split("|dS|/|S| = ")[1] for ln in out.splitlines() if "|dS|/|S|" in ln]
    assert len(history(run.stdout)) == 4 and "Lambda* (" in run.stdout and "Lambda* (" in multi.stdout
    assert history(multi.stdout) == history(run.stdout)
    J = np.load(one / "J0.npy")
    for rank in range(ranks):
        sh = Shard2D(rank, ranks, 8)
        lo, hi = sh.groups
        assert sh.r_dir == 1
        assert np.array_equal(np.load(many / f"J{rank}.npy"), J[lo:hi])
