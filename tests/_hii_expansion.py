"""A numpy restatement of the start-up expansion of HII regions (equiSources.f90:1035-1069: computeExpansionParameters :4395,
absoluteCoordinates :3011, findExpansion :4431, applyExpansion :4476): the yardstick of ftte_expand_hii_regions.

Every operation is a plain IEEE add, multiply, divide or square root in the reference's order, binary64 except where the reference
computes in single precision: the three tables of computeExpansionParameters, the literals, and findExpansion's shift
0.25 / (float(2**level) * float(nx)).  log10 and 10**x are the host's libm, as in ftte_expansion_parameters.
"""
import math

import numpy as np

F32 = lambda x: float(np.float32(x))  # noqa: E731  (a default-real literal widened)
PSI, MH, PC = F32(0.76), F32(1.6726231e-24), F32(3.08568025e18)
MARGIN = F32(1.0001)
LI = [F32(v) for v in (0.00000, 0.333333, 0.666667, 1.00000, 1.33333, 1.66667, 2.00000, 2.33333, 2.66667, 3.00000)]
LR = [F32(v) for v in (2.99506, 2.77808, 2.57210, 2.37683, 2.19731, 2.02898, 1.87315, 1.73656, 1.61294, 1.50202)]
LD = [F32(v) for v in (-0.0222764, 0.295050, 0.579490, 0.831870, 1.03717, 1.20892, 1.34321, 1.41970, 1.45725, 1.45667)]


def table_interval(nh):
    """the 1-based index i of computeExpansionParameters after the clamp, and whether nh lies below the table"""
    lognh = math.log10(nh)
    i = 1
    while lognh > LI[i - 1] and i < 10:
        i += 1
    return max(i, 2), lognh < LI[0]


def expansion_parameters(nh):
    """computeExpansionParameters(nh): (finalRadius [cm], densityCoefficient)"""
    nh = float(nh)
    lognh = math.log10(nh)
    i, below = table_interval(nh)
    tmp = (lognh - LI[i - 2]) / (LI[i - 1] - LI[i - 2])
    radius = math.pow(10.0, tmp * (LR[i - 1] - LR[i - 2]) + LR[i - 2]) * PC
    coef = math.pow(10.0, tmp * (LD[i - 1] - LD[i - 2]) + LD[i - 2]) / nh
    if below:
        tmp = (lognh + 6.0) / (LI[0] + 6.0)
        coef = math.pow(10.0, tmp * (LD[0] + 6.0) - 6.0) / nh
    return radius, coef


def leaf_paths(n, level):
    """The tree of a depth-first level list: per leaf its base cell (i, j, k), 0-based, and the children (a, b, c), 0 or 1, taken
    from the base cell down."""
    level = np.asarray(level)
    base, path = [], []
    cursor = 0

    def grow(depth, cell, taken):
        nonlocal cursor
        if level[cursor] == depth:
            base.append(cell)
            path.append(tuple(taken))
            cursor += 1
        else:
            assert level[cursor] > depth
            for a in range(2):
                for b in range(2):
                    for c in range(2):
                        grow(depth + 1, cell, taken + [(a, b, c)])

    for i in range(n):
        for j in range(n):
            for k in range(n):
                grow(0, (i, j, k), [])
    assert cursor == level.size
    return base, path


def call_sequence(base, path):
    """a leaf's call sequence as a star carries it: base indices 1..n, then child indices 1..2 per level"""
    seq = [base[0] + 1, base[1] + 1, base[2] + 1]
    for step in path:
        seq += [step[0] + 1, step[1] + 1, step[2] + 1]
    return seq


def leaf_centres(n, level):
    """findExpansion's xcell, ycell, zcell of every leaf: [ncell][3]"""
    base, path = leaf_paths(n, level)
    out = np.empty((len(base), 3))
    for q, (cell, taken) in enumerate(zip(base, path)):
        p = [(float(cell[a] + 1) - 0.5) / float(n) for a in range(3)]
        for lev, step in enumerate(taken):
            shift = float(np.float32(0.25) / (np.float32(2 ** lev) * np.float32(n)))
            p = [p[a] + shift if step[a] else p[a] - shift for a in range(3)]
        out[q] = p
    return out


def star_centre(n, base, taken):
    """absoluteCoordinates from (.5, .5, .5): xbase, ybase, zbase of a leaf"""
    p = [0.5, 0.5, 0.5]
    for step in reversed(taken):
        p = [0.5 * p[a] + 0.5 if step[a] else 0.5 * p[a] for a in range(3)]
    return [(float(np.float32(base[a])) + p[a]) / float(np.float32(n)) for a in range(3)]


def star_centres(n, level, src_cells):
    base, path = leaf_paths(n, level)
    return np.array([star_centre(n, base[int(c)], path[int(c)]) for c in src_cells]).reshape(-1, 3)


def rho_coef(n, level, box, rho, src_cells, params, centres=None):
    """rhoCoef of every leaf after findExpansion for all stars; params[nsrc][3] = finalRadius, densityCoefficient,
    sourceTotalHydrogenDensity"""
    rho = np.asarray(rho, np.float64)
    centres = leaf_centres(n, level) if centres is None else centres
    stars = star_centres(n, level, src_cells)
    nh = PSI * rho / MH
    coef = np.ones(rho.size)
    for (xb, yb, zb), (radius, dcoef, nh_src) in zip(stars, np.asarray(params, np.float64).reshape(-1, 3)):
        dx, dy, dz = xb - centres[:, 0], yb - centres[:, 1], zb - centres[:, 2]
        dist = box * np.sqrt(dx * dx + dy * dy + dz * dz)
        hit = (dist < radius) & (nh <= MARGIN * nh_src)
        coef[hit] = np.minimum(coef[hit], dcoef)
    return coef


def apply_expansion(coef, *fields):
    """applyExpansion: each field times rhoCoef where rhoCoef < 1"""
    lower = coef < 1.0
    return [np.where(lower, np.asarray(f, np.float64) * coef, np.asarray(f, np.float64)) for f in fields]


def parameters_of(rho, src_cells, fn=expansion_parameters):
    """[nsrc][3] from the host leaves' densities, as the call with params = NULL forms them"""
    out = np.empty((len(src_cells), 3))
    for s, c in enumerate(src_cells):
        nh = PSI * float(rho[int(c)]) / MH
        out[s, :2] = fn(nh)
        out[s, 2] = nh
    return out
