"""Host yardsticks of the accelerated source iteration -- test infrastructure only, nothing of the code under test.

probe_uniform / probe_tree: the diagonal of the Lambda operator by probing the oracle's sweep (S = 1 in one cell, 0 elsewhere, no
inflow, read J in that cell), every cell.  formula_uniform: the same number from its definition, segment by segment, with the
oracle's restatement of the device arithmetic.  iterate: the three iteration schemes with any sweep as a callable.
"""
from concurrent.futures import ThreadPoolExecutor

import numpy as np

import _oracle as O


def _probe(sweep, kappa, batch):
    """sweep(kappa_rep [m][ncell], src [m][ncell]) -> J [m][ncell]; the probes of one frequency group travel as `batch` groups."""
    nnu, ncell = kappa.shape
    jobs = [(g, lo, min(ncell, lo + batch)) for g in range(nnu) for lo in range(0, ncell, batch)]
    out = np.empty_like(kappa)

    def one(job):
        g, lo, hi = job
        m = hi - lo
        src = np.zeros((m, ncell))
        src[np.arange(m), np.arange(lo, hi)] = 1.0
        J = sweep(np.repeat(kappa[g:g + 1], m, axis=0), src)
        out[g, lo:hi] = J[np.arange(m), np.arange(lo, hi)]

    O.lib()
    with ThreadPoolExecutor(max_workers=O.oracle_threads()) as pool:
        list(pool.map(one, jobs))
    return out


def probe_uniform(n, kappa, box, phi, theta, w, batch=32):
    def sweep(kap, src):
        return O.sweep_uniform(n, kap, box, phi, theta, w, np.zeros(len(kap)), src=src, arith=O.ARITH_DEVICE)
    return _probe(sweep, np.ascontiguousarray(kappa, dtype=np.float64), batch)


def probe_tree(n, level, kappa, box, phi, theta, w, batch=32):
    def sweep(kap, src):
        return O.sweep_tree(n, level, kap, box, phi, theta, w, np.zeros(len(kap)), src=src, arith=O.ARITH_DEVICE)
    return _probe(sweep, np.ascontiguousarray(kappa, dtype=np.float64), batch)


def formula_uniform(n, kappa_at, cells, box, phi, theta, w):
    """The definition, for the cells `cells` (cell-array indices) of one group with opacities kappa_at: per direction the means
    of the cell's segments with Iin = 0, S = 1 (device arithmetic) added in the order xy, xz, yz, the cell mean, directions added
    in list order."""
    cells = np.asarray(cells)
    pos = np.stack([cells // (n * n), (cells // n) % n, cells % n])
    delta = box / float(n)
    out = np.zeros(len(cells))
    for p, t, wd in zip(phi, theta, w):
        pf, tf, izone = O.fold_direction(p, t)
        pats = O.layer_patterns(n, pf, tf)
        r1, r2 = O.rotate_indices(1, 1, 1, n, n, n, izone), O.rotate_indices(2, 1, 1, n, n, n, izone)
        axis = [a for a in range(3) if r1[a] != r2[a]][0]
        layer = pos[axis] if r2[axis] > r1[axis] else n - 1 - pos[axis]
        lens = np.array([[q.xy_len, q.xz_len if q.xz_active else 0.0, q.yz_len if q.yz_active else 0.0] for q in pats])
        nseg = np.array([1 + (1 if q.xz_active else 0) + (1 if q.yz_active else 0) for q in pats])
        active = np.array([[1, q.xz_active, q.yz_active] for q in pats]) != 0
        acc = np.zeros(len(cells))
        for s in range(3):
            tau = kappa_at * (delta * lens[layer, s])
            _, mean = O.device_segment_source(np.zeros(len(cells)), tau, 1.0)
            acc = np.where(active[layer, s], acc + mean, acc)
        term = np.empty(len(cells))
        for k in (1, 2, 3):
            sel = nseg[layer] == k
            if sel.any():
                term[sel] = O.device_cell_mean(acc[sel], k, wd)
        out = out + term
    return out


def ng_extrapolate(hist):
    """Ng's three-term extrapolation of one group's iterates hist = [y3, y2, y1, y0] (y0 the newest); None if singular."""
    y3, y2, y1, y0 = hist
    q1, q2, q3 = y0 - 2.0 * y1 + y2, y0 - y1 - y2 + y3, y0 - y1
    A1, B1, B2, C1, C2 = q1 @ q1, q1 @ q2, q2 @ q2, q1 @ q3, q2 @ q3
    det = A1 * B2 - B1 * B1
    if not np.isfinite(det) or det == 0.0 or abs(det) <= 1e-30 * abs(A1 * B2):
        return None
    a, b = (C1 * B2 - C2 * B1) / det, (C2 * A1 - C1 * B1) / det
    return (1.0 - a - b) * y0 + a * y1 + b * y2


def iterate(sweep, scheme, steps, eps, B, shape, diag=None, ng_start=4, ng_period=4, on_step=None):
    """scheme None | "diagonal" | "diagonal+ng"; sweep(S) -> J.  Returns (S, measures): the plain scheme's measure is
    max |dJ| / max |J|, the accelerated ones' max |dS| / max |S| of the operator update."""
    J = np.zeros(shape)
    S = (1.0 - eps) * J + eps * B
    hist, measures = [], []
    for k in range(1, steps + 1):
        if scheme is None:
            S = (1.0 - eps) * J + eps * B
            Jn = sweep(S)
            measures.append(np.abs(Jn - J).max() / np.abs(Jn).max())
            J = Jn
            state = (1.0 - eps) * J + eps * B
        else:
            J = sweep(S)
            Sn = S + (((1.0 - eps) * J + eps * B) - S) / (1.0 - (1.0 - eps) * diag)
            measures.append(np.abs(Sn - S).max() / np.abs(Sn).max())
            S = Sn
            if scheme == "diagonal+ng":
                hist = (hist + [S.copy()])[-4:]
                if k >= ng_start and (k - ng_start) % ng_period == 0 and len(hist) == 4:
                    S = S.copy()
                    for g in range(shape[0]):
                        y = ng_extrapolate([h[g] for h in hist])
                        if y is not None:
                            S[g] = y
                    hist = []
            state = S
        if on_step is not None:
            on_step(k, state)
    return state, measures
