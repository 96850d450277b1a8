"""A fixed, seeded slice of the three randomised scripts (fuzz_gpu.py, fuzz_hybrid_gpu.py, fuzz_fine_gpu.py) as part of the suite.

Each case is drawn from its own generator (case_rng(seed, case) in the script), so the slice is the same on every run and a
failing case can be re-run alone: python tests/<script> <case + 1> <seed> prints every case up to it, or make_case(seed, case)
and run_case from a Python prompt.  The uniform-grid cases compare with the oracle (device arithmetic); the refined ones with the
library's forest path of the whole tree, which the parity tests pin to the oracle.  All to 64 eps relative, and the refined ones
reproducible run to run."""
import numpy as np
import pytest

import fuzz_fine_gpu
import fuzz_gpu
import fuzz_hybrid_gpu

pytestmark = pytest.mark.gpu

SEED = 1
SUM_RTOL = 64 * np.finfo(np.float64).eps
UNIFORM_CASES, ALIGNED_CASES, UNIFORM_MAX_UPDATES = 10, 4, 2.5e7   # the oracle's host time bounds the uniform slice
HYBRID_CASES, FINE_CASES = 8, 8


def _uniform_slice():
    """The first UNIFORM_CASES cases of SEED whose oracle sweep stays under UNIFORM_MAX_UPDATES cell updates, and as many more of
    the following ones as it takes to hold ALIGNED_CASES of a size that is a multiple of 64 (accumulator pairs, one-launch forms)."""
    picked, aligned = [], 0
    for case in range(2000):
        c = fuzz_gpu.make_case(SEED, case)
        if fuzz_gpu.cost(c) > UNIFORM_MAX_UPDATES:
            continue
        a = c["n"] % 64 == 0
        if len(picked) < UNIFORM_CASES or (a and aligned < ALIGNED_CASES):
            picked.append(c)
            aligned += a
        if len(picked) >= UNIFORM_CASES and aligned >= ALIGNED_CASES:
            break
    return picked


def _report(script, c, line):
    return f"{script} seed {c['seed']} case {c['case']}:\n{line}"


def test_uniform_cases_against_the_oracle():
    import radiativetransfer_amd as rt
    cases = _uniform_slice()
    assert sum(c["n"] % 64 == 0 for c in cases) == ALIGNED_CASES and len(cases) <= UNIFORM_CASES + ALIGNED_CASES
    with rt.DiffuseTransfer() as eng:
        for c in cases:
            err, line = fuzz_gpu.run_case(eng, c)
            print(line)
            assert err <= SUM_RTOL, _report("fuzz_gpu.py", c, line)


@pytest.mark.parametrize("case", range(HYBRID_CASES))
def test_hybrid_cases_against_the_forest_path(case):
    c = fuzz_hybrid_gpu.make_case(SEED, case)
    err, ok, line = fuzz_hybrid_gpu.run_case(c)
    print(line)
    assert ok and err <= SUM_RTOL, _report("fuzz_hybrid_gpu.py", c, line)


@pytest.mark.parametrize("case", range(FINE_CASES))
def test_fine_block_cases_against_the_forest_path(case):
    c = fuzz_fine_gpu.make_case(SEED, case)
    err, ok, fine, line = fuzz_fine_gpu.run_case(c)
    print(line)
    assert ok and err <= SUM_RTOL, _report("fuzz_fine_gpu.py", c, line)


def test_fine_block_slice_reaches_the_fine_bricks():
    """At least some cases of the slice have a block the fine bricks may take (a cube of 32 or 64 base cells, no extra patch)."""
    assert sum(not fuzz_fine_gpu.make_case(SEED, case)["extra"] for case in range(FINE_CASES)) >= 4
