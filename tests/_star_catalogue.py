"""A numpy restatement of the star catalogue (equiSources.f90:746-769, :1169-1212): the yardstick of ftte_star_catalogue where no
golden file reaches -- large star sets, synthetic trees.

Every operation is the reference's, in binary64: the unit-cube coordinate (p - lo) / (hi - lo), int(x * n) with its remainder
x * float(n) - float(i), the descent by x >= 0.5 -> 2x - 1, else 2x.  Stars are merged by host leaf (np.unique), the sources come in
ascending leaf, first_star is the lowest star index with weight > 0.
"""
import numpy as np


def build_tree(n, level):
    """The tree of a depth-first level list as the library numbers it: nodes 0 .. n^3 - 1 the base cells (k fastest), the eight
    children of a refined node contiguous (4 a + 2 b + c).  Returns child0[nnode], leaf[nnode] (-1 where there is none), parent[nnode]."""
    level = np.asarray(level)
    nbase = n ** 3
    child0, leaf, parent = [-1] * nbase, [-1] * nbase, [-1] * nbase
    cursor = 0
    for b in range(nbase):
        stack = [(b, 0)]
        while stack:
            node, depth = stack.pop()
            if level[cursor] == depth:
                leaf[node] = cursor
                cursor += 1
            else:
                assert level[cursor] > depth
                c0 = len(child0)
                child0[node] = c0
                child0 += [-1] * 8
                leaf += [-1] * 8
                parent += [node] * 8
                stack += [(c0 + c, depth + 1) for c in range(7, -1, -1)]
    assert cursor == level.size
    return np.array(child0, np.int64), np.array(leaf, np.int64), np.array(parent, np.int64)


def locate(n, child0, leaf, xyz, lo=(0.0, 0.0, 0.0), hi=(1.0, 1.0, 1.0)):
    """star_cell[nstars]: the host leaf, -1 outside the box (0 <= int(x n) < n on every axis, int() truncating)"""
    xyz = np.asarray(xyz, np.float64).reshape(-1, 3)
    lo, hi = np.asarray(lo, np.float64), np.asarray(hi, np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        x = (xyz - lo) / (hi - lo)
        xn = x * float(n)
        inside = ((xn > -1.0) & (xn < float(n))).all(axis=1)
    out = np.full(len(xyz), -1, np.int64)
    x = x[inside]
    base = np.trunc(x * float(n)).astype(np.int64)
    p = x * float(np.float32(n)) - base.astype(np.float32).astype(np.float64)
    node = (base[:, 0] * n + base[:, 1]) * n + base[:, 2]
    live = child0[node] >= 0
    while live.any():
        h = (p[live] >= 0.5)
        p[live] = np.where(h, 2.0 * p[live] - 1.0, 2.0 * p[live])
        node[live] = child0[node[live]] + 4 * h[:, 0] + 2 * h[:, 1] + h[:, 2]
        live = child0[node] >= 0
    out[inside] = leaf[node]
    return out


def merge(star_cell, weight=None):
    """(cell, weight, first_star) of the sources: the leaves that hold weight > 0, ascending"""
    star_cell = np.asarray(star_cell, np.int64)
    weight = np.ones(len(star_cell), np.int64) if weight is None else np.asarray(weight, np.int64)
    star = np.flatnonzero((star_cell >= 0) & (weight > 0))
    cell, first, inverse = np.unique(star_cell[star], return_index=True, return_inverse=True)
    return cell, np.bincount(inverse, weights=weight[star], minlength=len(cell)).astype(np.int64), star[first]


def call_sequences(n, child0, leaf, parent):
    """per leaf (level, call sequence 1-based) from the tree's arrays"""
    out = [None] * int((leaf >= 0).sum())
    for node in np.flatnonzero(leaf >= 0):
        seq, at = [], int(node)
        while parent[at] >= 0:
            c = at - int(child0[parent[at]])
            seq = [(c >> 2) + 1, ((c >> 1) & 1) + 1, (c & 1) + 1] + seq
            at = int(parent[at])
        seq = [at // (n * n) + 1, (at // n) % n + 1, at % n + 1] + seq
        out[int(leaf[node])] = (len(seq) // 3 - 1, seq)
    return out


def location_keys(n, child0, leaf, parent):
    """the reference's location key of every leaf (:1177-1192)"""
    keys = np.empty(int((leaf >= 0).sum()), np.int64)
    for cell, (_, seq) in enumerate(call_sequences(n, child0, leaf, parent)):
        key = ((seq[0] - 1) * n + (seq[1] - 1)) * n + seq[2]
        for q in range(3, len(seq), 3):
            key = 10 * key + 4 * (seq[q] - 1) + 2 * (seq[q + 1] - 1) + seq[q + 2]
        keys[cell] = key
    return keys


def colliding_leaves(keys):
    """how many leaves share their key with another leaf"""
    _, inverse, count = np.unique(keys, return_inverse=True, return_counts=True)
    return int((count[inverse] > 1).sum())
