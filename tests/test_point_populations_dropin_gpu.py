"""fortran/ftte_stellar_transfer.f90 with ftteStarBatch > 1: stars collected into batches, their populations into slots, two calls per
batch -- and per star, in star order, what the per-star sequence (ftteStarBatch = 1) produces.  Run as the reference driver would
run it (tests/fortran/dropin_check on the reference's own tree and module arrays), once per setting."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DROPIN = os.path.join(ROOT, "tests", "fortran", "dropin_check")
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))

pytestmark = pytest.mark.gpu


def test_dropin_star_batches_equal_the_per_star_sequence(golden, tmp_path):
    import make_golden_point as M
    if not os.path.exists(DROPIN):
        # the binary links the reference's modules: without them it cannot exist; with them its absence is a broken build
        assert not os.path.isdir(os.path.join(ROOT, "oracle", "_ref")), "oracle/_ref is built but tests/fortran/dropin_check is not"
        pytest.skip("tests/fortran/dropin_check not built (needs oracle/_ref at build time)")
    g = golden("point10_refined_dust")
    n, level = int(g["n"]), g["level"]
    a_smc, wavelength, spec = M.synthetic_population()
    seqs, cursor = [], 0

    def grow(lvl, path):  # call sequences of the leaves, as readCellArray.f90:154-187 numbers them
        nonlocal cursor
        if level[cursor] == lvl:
            seqs.append(path)
            cursor += 1
        else:
            for a in (1, 2):
                for b in (1, 2):
                    for c in (1, 2):
                        grow(lvl + 1, path + [a, b, c])
    for i in range(1, n + 1):
        for j in range(1, n + 1):
            for k in range(1, n + 1):
                grow(0, [i, j, k])
    # eleven stars, one of weight 0 (skipped), in cells of five different metallicities: two of them shared by several stars that
    # are not neighbours in the list, all four brackets of the metallicity grid in use
    rng = np.random.default_rng(17)
    leaves = rng.choice(level.size, 11, replace=False)
    weights = rng.integers(1, 40, 11)
    weights[4] = 0
    abun2 = g["abun2"].astype(float).copy()
    metallicity = np.log10(float(abun2[0])) - 0.1 + np.arange(5.0)
    abun2[leaves] = 10.0 ** (metallicity[0] + np.array([0.1, 1.3, 0.1, 2.5, 0.7, 3.9, 1.3, 0.1, 2.5, 4.4, -3.0]))
    case = tmp_path / "case.bin"
    with open(case, "wb") as f:
        f.write(np.array([n, level.size, leaves.size, int(g["dust"])], "<i4").tobytes())
        f.write(np.array([float(g["box"])], "<f8").tobytes())
        f.write(level.astype("<i4").tobytes())
        for k in ("HI", "HeI", "HeII", "rho"):
            f.write(g[k].astype("<f8").tobytes())
        f.write(abun2.astype("<f8").tobytes())
        for leaf, weight in zip(leaves, weights):
            seq = seqs[int(leaf)]
            f.write(np.array([len(seq) // 3 - 1, int(weight)] + seq + [0] * (33 - len(seq)), "<i4").tobytes())
        f.write(np.asfortranarray(a_smc).tobytes(order="F"))
        f.write(np.asarray(wavelength, "<f8").tobytes())
        f.write(np.asfortranarray(spec).tobytes(order="F"))
        f.write(metallicity.astype("<f8").tobytes())
        f.write(np.array([int(g["iSpectrum"])], "<i4").tobytes())
        f.write(np.array([float(g["coefSpectrum"])], "<f8").tobytes())

    def run(batch):
        out = tmp_path / f"rates{batch}.bin"
        env = dict(os.environ)
        env.pop("FTTE_STAR_BATCH", None)
        if batch:
            env["FTTE_STAR_BATCH"] = str(batch)
        res = subprocess.run([DROPIN, "stellar", str(case), str(out)], capture_output=True, text=True, timeout=300, env=env)
        assert res.returncode == 0 and "dropin_check OK" in res.stdout, res.stdout + res.stderr
        return np.fromfile(out, "<f8").reshape(6, level.size), [ln for ln in res.stdout.splitlines() if ln.startswith("src:")]

    ref, lines = run(0)
    assert len(lines) == 10 and ref[0].sum() > 0
    scale = np.abs(ref).max(axis=1, keepdims=True)
    for batch in (4, 64):  # three batches with the last one short; one batch for all
        rates, got = run(batch)
        # the same deposits in another order of the atomics (the tolerance of test_many_sources_batches_and_linearity)
        assert np.all(np.abs(rates - ref) <= 1e-11 * np.abs(ref) + 1e-14 * scale), batch
        assert np.array_equal(rates == 0, ref == 0)
        # star number, level, neutral fraction, the star's own highestPixelLevel and weight as printed; fractions to the five decimals
        assert [ln.split()[:5] + ln.split()[-1:] for ln in got] == [ln.split()[:5] + ln.split()[-1:] for ln in lines], batch
        for a, b in zip(got, lines):
            assert np.allclose([float(x) for x in a.split()[5:12]], [float(x) for x in b.split()[5:12]], rtol=0, atol=2e-5)
