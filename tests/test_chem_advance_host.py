"""The time-dependent ionisation step (chem_advance_cell of radiativetransfer_amd/csrc/ftte_chem_math.h) on the host, without a GPU.

tests/host/chem_advance_check.cpp includes the header.  As a program it runs under AddressSanitizer and
UndefinedBehaviorSanitizer; as a small shared library without them (tests/_chem_advance.py) it gives these tests the host
evaluation, which is held against

  (a) the reference's start-up equilibrium (tests/golden/initial_refined.npz: its own compiled routine): a step of 1e40 s,
      twice, the self-shielding test taken anew the second time, in all 405 cells;
  (b) the header's own equilibrium bisection at the same rates (J-driven, without and with the point sources' rates);
  (c) an independent restatement of the step in numpy;
  (d) the closed form of hydrogen alone with constant recombination: first order in the step;
  (e) the invariants: outputs within the budget for over-full inputs, an empty cell fails, a tiny step changes nothing.

The bounds of (a) and (b) are 16 times the worst difference measured when the step was written, in units of the element's
density (DESIGN.md 3d'''): what separates the two sides is the rounding of two different closings of the same equations."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import _chem_advance as A

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "radiativetransfer_amd", "csrc")
HOST = os.path.join(ROOT, "tests", "host")

EPS = np.finfo(float).eps
WORST_A, WORST_B, CEILING = A.WORST_A, A.WORST_B, A.CEILING


def _table(g):
    return float(g["logtem0"]), float(g["logtem9"]), float(g["dlogtem"]), g["k"]


def _densities(rho):
    return A.PSI * rho / A.MH, (1.0 - A.PSI) * rho / A.MHE


def _chem_args(g, tab, krate, run_uvb):
    return (int(g["n"]), g["level"], float(g["box"]), g["rho"], g["tgas"], g["HI"], g["HeI"], g["HeII"], krate, run_uvb,
            g["J"] if run_uvb else None, g["ksi"] if run_uvb else None, None if run_uvb else g["uniform"],
            0.0 if run_uvb else float(g["threshold"]), *_table(tab))


def _worst(got, want, rho):
    nh, nhe = _densities(rho)
    return max((np.abs(got[0] - want[0]) / nh).max(), (np.abs(got[1] - want[1]) / nhe).max(), (np.abs(got[2] - want[2]) / nhe).max())


def test_step_under_asan_and_ubsan(tmp_path):
    gxx = shutil.which("g++")
    if not gxx:
        pytest.skip("no g++")
    exe = str(tmp_path / "chem_advance")
    cmd = [gxx, "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-I" + CSRC, os.path.join(HOST, "chem_advance_check.cpp"), "-o", exe]
    build = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    if build.returncode != 0 and ("asan" in build.stderr or "ubsan" in build.stderr) and "cannot find" in build.stderr:
        pytest.skip("sanitizer runtimes not installed")
    assert build.returncode == 0, build.stderr[-3000:]
    run = subprocess.run([exe], capture_output=True, text=True, timeout=600,
                         env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1"))
    assert run.returncode == 0, (run.stdout + run.stderr)[-4000:]
    assert "chem advance under the sanitizers: ok" in run.stdout and "ERROR" not in run.stderr


def test_long_step_lands_on_the_reference_equilibrium(golden):
    """(a)"""
    g, tab = golden("initial_refined"), golden("chem_uvb_refined")
    assert g["rho"].size == 405
    state = (g["HI"], g["HeI"], g["HeII"])
    for _ in range(2):
        out = A.advance(int(g["n"]), g["level"], float(g["box"]), g["rho"], g["tgas"], *state, None, False, None, None, g["uniform"],
                        float(g["threshold"]), *_table(tab), 1e40, 1)
        assert out[3] == 0
        state = out[:3]
    worst = _worst(state, (g["HI_out"], g["HeI_out"], g["HeII_out"]), g["rho"])
    print(f"(a) worst difference / element density {worst:.3e} over {g['rho'].size} cells, {out[4].mean():.1f} steps per cell")
    assert 16 * WORST_A <= CEILING
    assert worst <= 16 * WORST_A


@pytest.mark.parametrize("point", [False, True])
def test_long_step_lands_on_the_header_equilibrium(golden, point):
    """(b)"""
    g = golden("chem_uvb_refined")
    args = _chem_args(g, g, g["krate"] if point else None, True)
    got, want = A.advance(*args, 1e40, 1), A.equilibrium(*args)
    assert got[3] == 0 and want[3] == 0
    worst = _worst(got, want, g["rho"])
    print(f"(b) point rates {point}: worst difference / element density {worst:.3e}")
    assert 16 * WORST_B <= CEILING
    assert worst <= 16 * WORST_B


@pytest.mark.parametrize("name,mode", [("chem_uvb_refined", "J"), ("chem_uvb_refined", "J+point"), ("chem_uniform_background", "uniform"),
                                       ("initial_refined", "uniform")])
@pytest.mark.parametrize("dt,substeps", [(1e9, 1), (1e13, 3), (1e40, 1)])
def test_against_the_numpy_restatement(golden, name, mode, dt, substeps):
    """(c)"""
    g, tab = golden(name), golden("chem_uvb_refined")
    args = _chem_args(g, tab, g["krate"] if mode == "J+point" else None, mode != "uniform")
    got, mine = A.advance(*args, dt, substeps), A.advance_numpy(*args, dt, substeps)
    assert got[3] == 0 and mine[3].all()
    assert _worst(got, mine, g["rho"]) <= 4 * EPS
    assert np.array_equal(got[4], mine[4])


def _hydrogen_only(k2):
    """a table with recombination of HII alone, constant in temperature"""
    k = np.zeros((6, 2))
    k[1] = k2
    return 0.0, 20.0, 20.0, k


def test_first_order_in_the_step():
    """(d): with k1 = k3 = k4 = k5 = k6 = 0, helium neutral and no helium rates, x = HII/nh obeys dx/dt = G (1 - x) - A x^2 with
    A = k2 nh, that is dx/dt = -A (x - x+)(x - x-) with x+- the roots of A x^2 + G x - G; then y = (x - x+)/(x - x-) decays as
    exp(-A (x+ - x-) t), and x = (x+ - x- y)/(1 - y)"""
    k2, gamma, t_end = 2.59e-13, 1e-13, 2e13
    nh = np.array([1e-4, 1e-3, 1e-2, 1e-1, 1.0])
    rho = nh * A.MH / A.PSI
    nh, nhe = _densities(rho)
    nc = rho.size
    uniform = np.array([gamma / (4.0 * A.PI), 0.0, 0.0])
    G = 4.0 * A.PI * uniform[0]
    a = k2 * nh
    root = np.sqrt(G * G + 4.0 * G * a)
    xp, xm = (-G + root) / (2.0 * a), (-G - root) / (2.0 * a)
    E = (0.0 - xp) / (0.0 - xm) * np.exp(-a * (xp - xm) * t_end)
    exact = (xp - xm * E) / (1.0 - E)
    assert np.all((exact > 0.3) & (exact < 1.0))
    err = {}
    for sub in (16, 32, 64, 128, 256, 512):
        HI, HeI, HeII, status, steps, _ = A.advance(1, np.zeros(nc, np.int32), 1e22, rho, np.full(nc, 1e4), nh, nhe, np.zeros(nc), None, False, None,
                                                    None, uniform, 0.0, *_hydrogen_only(k2), t_end, sub)
        assert status == 0
        assert np.array_equal(HeI, nhe) and np.all(HeII == 0.0)
        err[sub] = np.abs((nh - HI) / nh - exact)
    for sub in (16, 32, 64, 128, 256):
        ratio = err[2 * sub] / err[sub]
        print(f"(d) substeps {sub}: error {err[sub].max():.3e}, err(2N)/err(N) {ratio.min():.4f} .. {ratio.max():.4f}")
        assert np.all((ratio >= 0.4) & (ratio <= 0.6))


def test_outputs_stay_within_the_budget(golden):
    """(e): over-full and negative incoming species, every rate mode, short and long steps"""
    g = golden("chem_uvb_refined")
    rng = np.random.default_rng(5)
    nc = g["rho"].size
    nh, nhe = _densities(g["rho"])
    HI, HeI, HeII = nh * rng.uniform(-0.1, 1.5, nc), nhe * rng.uniform(-0.1, 1.5, nc), nhe * rng.uniform(-0.1, 1.5, nc)
    u = golden("chem_uniform_background")
    for krate, run_uvb in ((None, True), (g["krate"], True), (g["krate"], False)):
        for dt, sub in ((1e7, 1), (1e12, 4), (1e16, 2), (1e40, 1)):
            out = A.advance(int(g["n"]), g["level"], float(g["box"]), g["rho"], g["tgas"], HI, HeI, HeII, krate, run_uvb, g["J"], g["ksi"], u["uniform"],
                            float(u["threshold"]), *_table(g), dt, sub)
            assert out[3] == 0
            assert np.all((out[0] >= 0) & (out[0] <= nh * (1 + A.SLACK)))
            assert np.all((out[1] >= 0) & (out[2] >= 0) & (out[1] + out[2] <= nhe * (1 + A.SLACK)))


def test_an_empty_cell_fails(golden):
    """(e)"""
    g = golden("chem_uvb_refined")
    rho = g["rho"].copy()
    rho[7] = 0.0
    args = list(_chem_args(g, g, None, True))
    args[3] = rho
    assert A.advance(*args, 1e13, 1)[3] == 8
    assert not A.advance_numpy(*args, 1e13, 1)[3][7]


def test_a_tiny_step_leaves_the_clipped_state(golden):
    """(e)"""
    g = golden("chem_uvb_refined")
    args = _chem_args(g, g, g["krate"], True)
    nh, nhe, a, b, d = A.clip(g["rho"], g["HI"], g["HeI"], g["HeII"])
    assert np.any(g["HI"] > nh)      # the golden holds cells over their budget
    for dt in (1e-30, 1e-10):
        out = A.advance(*args, dt, 1)
        assert out[3] == 0
        assert np.all(np.abs(out[0] - a) <= 4 * EPS * nh) and np.all(np.abs(out[1] - b) <= 4 * EPS * nhe) and np.all(np.abs(out[2] - d) <= 4 * EPS * nhe)
