#!/usr/bin/env python3
"""Golden vectors for the star catalogue (equiSources.f90:746-769, :1169-1212, :1282-1293), produced by the reference's own compiled
lines: the unit-cube coordinates and localizeSplitContinuationCell (:750-757, :3049-3118), localizeCellFromStar (:2597-2620), the
location key, sortStellarParticles (utilities.f90:11) and the merge of degenerate particles (:1172-1211), and the metallicity
bracket (:1282-1293).

    python -m radiativetransfer_amd.build && make -C oracle ref && python tests/golden/make_golden_catalogue.py

oracle/ stays as it is: like make_golden_expansion.py this script lifts the routines by line range into a module and the blocks of
the main program into a small generated driver (which grows the tree from the level list, each leaf remembering its index in an
unused field), compiles them and the reference's utilities.f90 with the oracle's compiler and flags against the definitionsModule
object that `make -C oracle ref` leaves in oracle/_ref/ -- all in a temporary directory that is deleted afterwards.  Each star's
input index travels through the sort in the unused field xpos of starType.  Only the .npz files (data) are written into the tree:

  catalogue_refined12.npz  the tree of expansion_refined.npz (12^3, levels 0 to 2; 12 is no power of two, so x*n rounds), a box
                           with corners that are no round numbers, about 3 000 stars in base and refined leaves, several per leaf,
                           weights 0, 1 and more; stars close to faces and child midplanes; and a small `collide_*` set in two
                           leaves that share the reference's location key
  catalogue_uniform16.npz  16^3 uniform (faces exactly representable), about 500 stars: 200 in one leaf, stars exactly on faces and
                           on the midplanes of cells, at 0, -0.0 and nextafter(1, 0)
  catalogue_ingested6.npz  the tree and abun2 of ingest6_three_levels_metals_velocities.npz, about 300 stars and a metallicity grid
                           of five nodes: abun2 below 1e-20, inside every interval and beyond both ends

The reference alone decides whether a star set qualifies: no two host leaves of a main set share a location key (else its merge
is no per-leaf merge; the stars that would are taken out by the keys the reference computed and the set is run again), no
log10(abun2) lies within 4 ulp of a metallicity node, every star handed over is inside the box (the reference indexes out of
bounds otherwise).  Stars outside are appended afterwards (`outside_xyz`, expected star_cell -1).

Per star: star_level, star_position (call sequence, zero-padded), star_leaf (host leaf, 0-based), star_key; after the merge: merged_leaf /
merged_weight (the leaves with weight > 0 and their sums, ascending leaf) and nSources; per survivor (ascending leaf): iMetal,
coefMetal, abun2.  The collide set holds the same with the prefix collide_, its merged_* being what the REFERENCE returns (the
survivor's leaf and the weight of both leaves), and collide_leaf_cell / collide_leaf_weight the per-leaf sums.  The files are written
with fixed zip timestamps, so a rerun reproduces them byte for byte.
"""
import os
import shutil
import struct
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)
from make_golden_initial import FC, FFLAGS, REF_BUILD, REFERENCE, save  # noqa: E402

MAXPOS = 33  # splitContinuationCallSequence, definitionsModule.f90:278

DRIVER_HEAD = r"""
! equiSources.f90:750-757, :1172-1211 and :1282-1293 on a cell array and a star list handed over in a stream file (generated; see
! make_golden_catalogue.py)
! case: int32 n, ncell, nStars ; real64 lo(3), hi(3) ; int32 level(ncell) ; real64 abun2(ncell) ; real64 xyz(3,nStars) ;
!       int32 weight(nStars) ; real64 metallicity(5)
! out:  int32 level(nStars), position(33,nStars), leaf(nStars), leafFromSequence(nStars) ; int64 key(nStars) ;
!       int32 order(nStars), mergedWeight(nStars), nSources ; per survivor int32 star, leaf, weight, iMetal ; real64 coefMetal, abun2
program catalogue_harness
  use definitions
  use utilities
  use catExtract
  implicit none
  integer :: n, ncell, nStars, cursor, i, j, k, nx, ny, nz, iStar, iref, itmp, iMetal   ! (nSources is the module's)
  integer, allocatable :: lev(:), w(:), slev(:), spos(:,:), sleaf(:), sleaf2(:), order(:), mw(:)
  integer, allocatable :: vstar(:), vleaf(:), vweight(:), vmetal(:)
  integer*8, allocatable :: skey(:)
  real(kind=RealKind), allocatable :: ab(:), xyz(:,:), vcoef(:), vabun(:)
  real(kind=RealKind) :: tmp, tmp1, tmp2, tmp3, xa, xb, ya, yb, za, zb, coefMetal, lo(3), hi(3)
  type(starType), dimension(:), pointer :: star
  type(starType), pointer :: currentStar, nextStar
  character(len=512) :: caseName, outName

  call get_command_argument(1, caseName)
  call get_command_argument(2, outName)
  open(11, file=trim(caseName), access='stream', form='unformatted', status='old')
  read(11) n, ncell, nStars
  read(11) lo, hi
  allocate(lev(ncell), ab(ncell), xyz(3,nStars), w(nStars), star(nStars))
  allocate(slev(nStars), spos(33,nStars), sleaf(nStars), sleaf2(nStars), skey(nStars), order(nStars), mw(nStars))
  read(11) lev
  read(11) ab
  read(11) xyz
  read(11) w
  read(11) metallicity
  close(11)
  nx = n ; ny = n ; nz = n
  xa = lo(1) ; ya = lo(2) ; za = lo(3)
  xb = hi(1) ; yb = hi(2) ; zb = hi(3)

  baseGrid%refined = .true.
  baseGrid%level = -1
  allocate(baseGrid%cell(n,n,n))
  cursor = 0
  do i = 1, n
     do j = 1, n
        do k = 1, n
           baseGrid%cell(i,j,k)%parent => baseGrid
           call growCell(baseGrid%cell(i,j,k), 0)
        enddo
     enddo
  enddo
  if (cursor /= ncell) stop 'catalogue_harness: level list does not describe a tree of ncell leaves'

  spos = 0
  do iStar = 1, nStars
     currentStar => star(iStar)
     tmp1 = xyz(1,iStar)
     tmp2 = xyz(2,iStar)
     tmp3 = xyz(3,iStar)
"""

DRIVER_MID = r"""
     currentStar%weight = w(iStar)
     currentStar%xpos = dble(iStar)
     slev(iStar) = currentStar%level
     spos(1:3*currentStar%level+3,iStar) = currentStar%position
     sleaf(iStar) = nint(splitContinuationCell%tgas) - 1
     i = currentStar%position(1)
     j = currentStar%position(2)
     k = currentStar%position(3)
     call localizeCellFromStar(baseGrid%cell(i,j,k),currentStar)
     sleaf2(iStar) = nint(currentStar%hostCell%tgas) - 1
  enddo
"""

DRIVER_TAIL = r"""
  allocate(vstar(nSources), vleaf(nSources), vweight(nSources), vmetal(nSources), vcoef(nSources), vabun(nSources))
  cursor = 0
  do iStar = 1, nStars
     currentStar => star(iStar)
     order(iStar) = nint(currentStar%xpos) - 1
     mw(iStar) = currentStar%weight
     if (currentStar%weight.gt.0) then
        i = currentStar%position(1)
        j = currentStar%position(2)
        k = currentStar%position(3)
        call localizeCellFromStar(baseGrid%cell(i,j,k),currentStar)
"""

DRIVER_END = r"""
        cursor = cursor + 1
        vstar(cursor) = nint(currentStar%xpos) - 1
        vleaf(cursor) = nint(currentStar%hostCell%tgas) - 1
        vweight(cursor) = currentStar%weight
        vmetal(cursor) = iMetal
        vcoef(cursor) = coefMetal
        vabun(cursor) = currentStar%hostCell%abun2
     endif
  enddo
  if (cursor /= nSources) stop 'catalogue_harness: survivors and nSources differ'

  open(12, file=trim(outName), access='stream', form='unformatted', status='replace')
  write(12) slev, spos, sleaf, sleaf2
  write(12) skey
  write(12) order, mw, nSources
  write(12) vstar, vleaf, vweight, vmetal
  write(12) vcoef, vabun
  close(12)

contains

  recursive subroutine growCell(c, level)
    type(zoneType), target :: c
    integer, intent(in) :: level
    integer :: a, b, d
    cursor = cursor + 1
    if (cursor > ncell) stop 'catalogue_harness: ran past the end of the level list'
    nullify(c%cell)
    c%level = int(level,1)
    if (lev(cursor) == level) then
       c%refined = .false.
       c%abun2 = ab(cursor)
       c%tgas = dble(cursor)
    else if (lev(cursor) > level) then
       cursor = cursor - 1
       c%refined = .true.
       allocate(c%cell(2,2,2))
       do a = 1, 2
          do b = 1, 2
             do d = 1, 2
                c%cell(a,b,d)%parent => c
                call growCell(c%cell(a,b,d), level+1)
             enddo
          enddo
       enddo
    else
       stop 'catalogue_harness: level list is not depth-first'
    endif
  end subroutine growCell

end program catalogue_harness
"""


def build_harness(tmp):
    lines = open(os.path.join(REFERENCE, "equiSources.f90")).read().split("\n")
    lift = lambda a, b: lines[a - 1:b]  # noqa: E731  (sed -n 'a,bp')
    mod = ["module catExtract", "  use definitions", "contains", *lift(2597, 2620), *lift(3049, 3118), "end module catExtract", ""]
    with open(os.path.join(tmp, "catExtract.f90"), "w") as f:
        f.write("\n".join(mod))
    # the keys as the reference computed them, in input order, are picked up between the key loop (:1172-1194) and the sort (:1196)
    keys = ["  do iStar = 1, nStars", "     skey(iStar) = star(iStar)%location", "  enddo"]
    driver = [DRIVER_HEAD, *lift(750, 757), DRIVER_MID, *lift(1172, 1194), *keys, *lift(1196, 1211), DRIVER_TAIL, *lift(1282, 1293),
              DRIVER_END]
    with open(os.path.join(tmp, "catalogue_harness.f90"), "w") as f:
        f.write("\n".join(driver))
    common = [FC, *FFLAGS, "-w", "-module-dir", tmp, "-I", REF_BUILD]
    subprocess.check_call([*common, "-c", os.path.join(REFERENCE, "utilities.f90"), "-o", os.path.join(tmp, "utilities.o")])
    subprocess.check_call([*common, "-c", os.path.join(tmp, "catExtract.f90"), "-o", os.path.join(tmp, "catExtract.o")])
    exe = os.path.join(tmp, "catalogue_harness")
    subprocess.check_call([*common, os.path.join(tmp, "catalogue_harness.f90"), os.path.join(tmp, "catExtract.o"),
                           os.path.join(tmp, "utilities.o"), os.path.join(REF_BUILD, "definitionsModule.o"), "-o", exe])
    return exe


def write_case(path, n, level, abun2, lo, hi, xyz, weight, metallicity):
    """the stream file the harness and fortran/ftte_demo_catalogue read"""
    with open(path, "wb") as f:
        f.write(struct.pack("<3i", n, len(level), len(xyz)))
        f.write(np.asarray(lo, "<f8").tobytes() + np.asarray(hi, "<f8").tobytes())
        f.write(np.asarray(level, "<i4").tobytes())
        f.write(np.asarray(abun2, "<f8").tobytes())
        f.write(np.ascontiguousarray(xyz, "<f8").tobytes())   # [nStars][3] = the Fortran array xyz(3,nStars)
        f.write(np.asarray(weight, "<i4").tobytes())
        f.write(np.asarray(metallicity, "<f8").tobytes())


def run_reference(exe, tmp, n, level, abun2, lo, hi, xyz, weight, metallicity):
    ns = len(xyz)
    case, out = os.path.join(tmp, "case.bin"), os.path.join(tmp, "out.bin")
    if os.path.exists(out):
        os.remove(out)
    write_case(case, n, level, abun2, lo, hi, xyz, weight, metallicity)
    res = subprocess.run([exe, case, out], capture_output=True, text=True)
    if res.returncode != 0 or not os.path.exists(out):
        raise RuntimeError(f"the reference stopped: {res.stdout[-800:]} {res.stderr[-500:]}")
    raw = open(out, "rb").read()
    at = 0

    def take(dtype, count):
        nonlocal at
        a = np.frombuffer(raw, dtype=dtype, count=count, offset=at).copy()
        at += a.nbytes
        return a

    r = dict(level=take("<i4", ns), position=take("<i4", MAXPOS * ns).reshape(ns, MAXPOS), leaf=take("<i4", ns),
             leaf_from_sequence=take("<i4", ns), key=take("<i8", ns), order=take("<i4", ns), sorted_weight=take("<i4", ns))
    nsrc = int(take("<i4", 1)[0])
    r.update(nSources=nsrc, surv_star=take("<i4", nsrc), surv_leaf=take("<i4", nsrc), surv_weight=take("<i4", nsrc),
             surv_iMetal=take("<i4", nsrc), surv_coefMetal=take("<f8", nsrc), surv_abun2=take("<f8", nsrc))
    assert at == len(raw)
    assert np.array_equal(r["leaf"], r["leaf_from_sequence"]), "localizeCellFromStar finds the leaf localizeSplitContinuationCell found"
    assert np.array_equal(np.sort(r["order"]), np.arange(ns)), "the input indices came through the sort"
    return r


def colliding_stars(r):
    """stars whose host leaf shares its location key with another host leaf of the set, by the reference's own keys and leaves"""
    pairs = np.unique(np.stack([r["key"], r["leaf"].astype(np.int64)], axis=1), axis=0)
    keys, count = np.unique(pairs[:, 0], return_counts=True)
    return np.isin(r["key"], keys[count > 1])


def fixture(prefix, r, xyz, weight):
    """the arrays of one star set; the survivors in ascending leaf"""
    by_leaf = np.argsort(r["surv_leaf"], kind="stable")
    maxpos = 3 * (int(r["level"].max()) + 1) if len(xyz) else 3
    g = {"xyz": np.ascontiguousarray(xyz, np.float64), "weight": np.asarray(weight, np.int32), "star_level": r["level"],
         "star_position": np.ascontiguousarray(r["position"][:, :maxpos]), "star_leaf": r["leaf"].astype(np.int64), "star_key": r["key"],
         "nSources": np.int64(r["nSources"]), "merged_leaf": r["surv_leaf"][by_leaf].astype(np.int64),
         "merged_weight": r["surv_weight"][by_leaf], "merged_star": r["surv_star"][by_leaf].astype(np.int64),
         "iMetal": r["surv_iMetal"][by_leaf], "coefMetal": r["surv_coefMetal"][by_leaf], "abun2_src": r["surv_abun2"][by_leaf]}
    return {prefix + k: v for k, v in g.items()}


def check_main(r, weight, metallicity):
    assert not colliding_stars(r).any(), "no two host leaves of the main set share a location key"
    # with distinct keys the reference's merge is a per-leaf merge: one survivor per leaf, carrying the leaf's sum
    leaves, inverse = np.unique(r["leaf"], return_inverse=True)
    sums = np.bincount(inverse, weights=weight).astype(np.int64)
    assert len(set(r["surv_leaf"].tolist())) == r["nSources"] == int((sums > 0).sum())
    assert np.array_equal(np.sort(r["surv_leaf"]), leaves[sums > 0])
    assert np.array_equal(r["surv_weight"][np.argsort(r["surv_leaf"])], sums[sums > 0])
    logs = np.log10(r["surv_abun2"][r["surv_abun2"] > np.float32(1e-20)])
    for node in metallicity:
        assert (np.abs(logs - node) > 4 * np.spacing(abs(node))).all(), "no log10(abun2) within 4 ulp of a metallicity node"
    assert len(leaves) < len(r["leaf"]), "several stars per leaf"


def outside_stars(lo, hi):
    lo, hi = np.asarray(lo), np.asarray(hi)
    mid, ext = 0.5 * (lo + hi), hi - lo
    rows = [[hi[0], mid[1], mid[2]], [mid[0], hi[1], mid[2]], [mid[0], mid[1], hi[2]],                      # 1.0 is outside
            [lo[0] - 0.25 * ext[0], mid[1], mid[2]], [mid[0], lo[1] - 3 * ext[1], mid[2]], [mid[0], mid[1], hi[2] + ext[2]],
            [np.nan, mid[1], mid[2]], [mid[0], np.inf, mid[2]], [mid[0], mid[1], -np.inf], [1e300, mid[1], mid[2]]]
    return np.array(rows)


def main():
    if not os.path.exists(os.path.join(REF_BUILD, "definitionsModule.o")):
        sys.exit("build the reference's modules first: make -C oracle ref")
    tmp = tempfile.mkdtemp()
    try:
        exe = build_harness(tmp)
        flat5 = np.log10(np.array([0.0004, 0.004, 0.008, 0.020, 0.050], np.float32).astype(np.float64))  # :844-845

        # (1) refined, 12^3 base
        rng = np.random.default_rng(746)
        e = np.load(os.path.join(HERE, "expansion_refined.npz"))
        n, level = int(e["n"]), e["level"].astype(np.int32)
        abun2 = 10 ** rng.uniform(-4.5, -1.0, level.size)
        lo, hi = np.array([-1.37, 0.21, 10.013]), np.array([2.55, 3.19, 14.407])
        u = rng.uniform(0, 1, (2200, 3))
        u = np.concatenate([u, u[rng.integers(0, 2200, 900)] + rng.uniform(-2e-3, 2e-3, (900, 3))])   # company in the same leaf
        cells = rng.integers(0, n, (120, 3))
        near = (cells + rng.choice([0.0, 0.25, 0.5, 0.75], (120, 3))) / n                             # faces, midplanes of children
        u = np.clip(np.concatenate([u, near]), 0.0, np.nextafter(1.0, 0.0))
        xyz = lo + u * (hi - lo)
        xyz = xyz[(((xyz - lo) / (hi - lo)) * n < n).all(axis=1) & ((xyz - lo) / (hi - lo) >= 0).all(axis=1)]
        weight = rng.choice([0, 1, 1, 1, 2, 3, 5], len(xyz)).astype(np.int32)
        r = run_reference(exe, tmp, n, level, abun2, lo, hi, xyz, weight, flat5)
        bad = colliding_stars(r)
        assert bad.any(), "the candidates reach leaves that share a key"
        # the collide set: the stars of one colliding pair of leaves
        key = r["key"][bad][0]
        pick = r["key"] == key
        assert len(set(r["leaf"][pick].tolist())) == 2
        cx, cw = xyz[pick], np.maximum(weight[pick], 1)
        cx = np.concatenate([cx, cx + 1e-9]); cw = np.concatenate([cw, cw + 1])
        rc = run_reference(exe, tmp, n, level, abun2, lo, hi, cx, cw, flat5)
        assert len(set(rc["leaf"].tolist())) == 2 and len(set(rc["key"].tolist())) == 1 and rc["nSources"] == 1
        xyz, weight = xyz[~bad], weight[~bad]
        r = run_reference(exe, tmp, n, level, abun2, lo, hi, xyz, weight, flat5)
        check_main(r, weight, flat5)
        assert set(r["level"].tolist()) == {0, 1, 2} and {0, 1} <= set(weight.tolist()) and weight.max() > 1
        g = dict(n=n, level=level, abun2=abun2, lo=lo, hi=hi, metallicity=flat5, outside_xyz=outside_stars(lo, hi))
        g.update(fixture("", r, xyz, weight))
        g.update(fixture("collide_", rc, cx, cw))
        leaves, inverse = np.unique(rc["leaf"], return_inverse=True)
        g["collide_leaf_cell"], g["collide_leaf_weight"] = leaves.astype(np.int64), np.bincount(inverse, weights=cw).astype(np.int32)
        print(f"catalogue_refined12: {len(xyz)} stars, {r['nSources']} sources, {int(bad.sum())} candidates in colliding leaves left out")
        save("catalogue_refined12", g)

        # (2) uniform 16^3, the unit box: every face and midplane is exact
        rng = np.random.default_rng(747)
        n, level = 16, np.zeros(16 ** 3, np.int32)
        abun2 = 10 ** rng.uniform(-4.5, -1.0, level.size)
        lo, hi = np.zeros(3), np.ones(3)
        last = np.nextafter(1.0, 0.0)
        crowd = (np.array([5, 9, 2]) + rng.uniform(0, 1, (200, 3))) / n
        faces = rng.integers(0, n, (60, 3)) / n
        mids = (rng.integers(0, n, (60, 3)) + 0.5) / n
        edge = np.array([[0.0, 0.0, 0.0], [-0.0, -0.0, -0.0], [last, last, last], [-0.0, 0.5, last], [last, 0.0, -0.0], [0.0, last, 0.5]])
        xyz = np.concatenate([crowd, faces, mids, edge, rng.uniform(0, 1, (180, 3))])
        weight = np.ones(len(xyz), np.int32)
        r = run_reference(exe, tmp, n, level, abun2, lo, hi, xyz, weight, flat5)
        check_main(r, weight, flat5)
        assert np.bincount(r["leaf"]).max() >= 200
        g = dict(n=n, level=level, abun2=abun2, lo=lo, hi=hi, metallicity=flat5, outside_xyz=outside_stars(lo, hi))
        g.update(fixture("", r, xyz, weight))
        print(f"catalogue_uniform16: {len(xyz)} stars, {r['nSources']} sources")
        save("catalogue_uniform16", g)

        # (3) the tree and abun2 the reference's ingest built, a metallicity grid of five nodes inside the range of its abun2
        rng = np.random.default_rng(748)
        s = np.load(os.path.join(HERE, "ingest6_three_levels_metals_velocities.npz"))
        n, level, abun2 = int(s["out_n"]), s["out_level"].astype(np.int32), s["out_abun2"].astype(np.float64)
        lo, hi = np.array([0.0, -30.0, 5.0]), np.array([60.0, 30.0, 65.0])
        metallicity = np.array([-3.6, -3.0, -2.6, -2.3, -1.9])
        u = rng.uniform(0, 1, (220, 3))
        u = np.clip(np.concatenate([u, u[rng.integers(0, 220, 90)] + rng.uniform(-4e-3, 4e-3, (90, 3))]), 0.0, last)
        xyz = lo + u * (hi - lo)
        xyz = xyz[(((xyz - lo) / (hi - lo)) * n < n).all(axis=1) & ((xyz - lo) / (hi - lo) >= 0).all(axis=1)]
        weight = rng.choice([1, 1, 2], len(xyz)).astype(np.int32)
        r = run_reference(exe, tmp, n, level, abun2, lo, hi, xyz, weight, metallicity)
        bad = colliding_stars(r)
        xyz, weight = xyz[~bad], weight[~bad]
        r = run_reference(exe, tmp, n, level, abun2, lo, hi, xyz, weight, metallicity)
        check_main(r, weight, metallicity)
        assert set(r["level"].tolist()) == {0, 1, 2}
        logs = np.where(r["surv_abun2"] > np.float32(1e-20), np.log10(np.maximum(r["surv_abun2"], 1e-300)), -20.0)
        assert (r["surv_abun2"] <= np.float32(1e-20)).any() and (logs > metallicity[-1]).any()
        assert ((logs < metallicity[0]) & (logs > -20)).any(), "beyond both ends of the grid"
        for a, b in zip(metallicity[:-1], metallicity[1:]):
            assert ((logs > a) & (logs < b)).any(), "abun2 inside every interval"
        assert set(r["surv_iMetal"].tolist()) == {1, 2, 3, 4} and r["surv_coefMetal"].min() == 0.0 and r["surv_coefMetal"].max() == 1.0
        g = dict(n=n, level=level, abun2=abun2, lo=lo, hi=hi, metallicity=metallicity, outside_xyz=outside_stars(lo, hi),
                 box=np.float64(s["out_box"]), HI=s["out_HI"].astype(np.float64), HeI=s["out_HeI"].astype(np.float64),
                 HeII=s["out_HeII"].astype(np.float64), rho=s["out_rho"].astype(np.float64))
        g.update(fixture("", r, xyz, weight))
        print(f"catalogue_ingested6: {len(xyz)} stars, {r['nSources']} sources, {int(bad.sum())} candidates in colliding leaves left out")
        save("catalogue_ingested6", g)
    finally:
        shutil.rmtree(tmp)


if __name__ == "__main__":
    main()
