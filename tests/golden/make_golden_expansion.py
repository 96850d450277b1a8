#!/usr/bin/env python3
"""Golden vectors for the start-up expansion of HII regions (equiSources.f90:1035-1069), produced by the reference's own compiled
lines: computeExpansionParameters (:4395), findExpansion (:4431) and applyExpansion (:4476) with localizeCellFromStar (:2597) and
absoluteCoordinates (:3011).

    python -m radiativetransfer_amd.build && make -C oracle ref && python tests/golden/make_golden_expansion.py

oracle/ stays as it is: like make_golden_initial.py this script lifts the routines by line range into a module, writes a small
driver next to it that grows the tree from the level list (rhoCoef = 1, level set) and replays :1038-1068 for the listed stars,
and compiles both with the oracle's compiler and flags against the definitionsModule object that `make -C oracle ref` leaves in
oracle/_ref/ -- all in a temporary directory that is deleted afterwards.  Only the .npz files (data) are written into the tree:

  expansion_refined.npz    12^3 base cells (no power of two: findExpansion's single-precision shift rounds), scattered refinement
                           to level 2, box 3 kpc, nH log-uniform over 1e-3 .. 10^3.5 cm^-3, 300 stars in base and refined leaves,
                           some sharing a leaf; host-cell densities in every table interval, on a table node, below 1, below 1e-6
                           (coefficient above 1) and above 1e3
  expansion_uniform16.npz  16^3 uniform, box 4 kpc, 40 stars
  expansion_ingested.npz   the tree of ingest6_three_levels_metals_velocities.npz with its own fields, the box rescaled to 60 kpc so
                           that the radii span cells, 12 stars

Each holds the inputs (n, level, box, rho, HI, HeI, HeII, the stars' call sequences and host cells), per star the reference's
finalRadius, densityCoefficient, sourceTotalHydrogenDensity (`params`) and xbase, ybase, zbase (`centres`), and per leaf rho_coef,
rho_out, HI_out, HeI_out, HeII_out.  The files are written with fixed zip timestamps, so a rerun reproduces them byte for byte.
"""
import math
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
import _hii_expansion as X  # noqa: E402
from make_golden_initial import FC, FFLAGS, REF_BUILD, REFERENCE, save  # noqa: E402
from radiativetransfer_amd import synthetic  # noqa: E402

KPC = 1.0e3 * X.PC

DRIVER = r"""
! equiSources.f90:1038-1068 on a cell array handed over in a stream file (generated; see make_golden_expansion.py)
! case: int32 n, ncell, nstars, maxpos ; real64 box ; int32 level(ncell) ; real64 f(ncell,4) = rho, HI, HeI, HeII ;
!       int32 starLevel(nstars) ; int32 starPosition(maxpos,nstars)
! out:  real64 s(nstars,6) = finalRadius, densityCoefficient, sourceTotalHydrogenDensity, xbase, ybase, zbase ;
!       real64 c(ncell,5) = rhoCoef, rho, HI, HeI, HeII
program expansion_harness
  use definitions
  use expExtract
  implicit none
  integer :: n, ncell, ns, maxpos, cursor, i, j, k, iStar
  integer, allocatable :: lev(:), slev(:), spos(:,:)
  real(kind=RealKind), allocatable :: f(:,:), outv(:,:), sout(:,:)
  real(kind=RealKind) :: box
  type(starType), allocatable, target :: st(:)
  type(starType), pointer :: currentStar
  type(pointType) :: startingPoint
  character(len=512) :: caseName, outName

  call get_command_argument(1, caseName)
  call get_command_argument(2, outName)
  open(11, file=trim(caseName), access='stream', form='unformatted', status='old')
  read(11) n, ncell, ns, maxpos
  read(11) box
  allocate(lev(ncell), f(ncell,4), outv(ncell,5), slev(ns), spos(maxpos,ns), sout(ns,6), st(ns))
  read(11) lev
  read(11) f
  read(11) slev
  read(11) spos
  close(11)
  physicalBoxSize = box

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
  if (cursor /= ncell) stop 'expansion_harness: level list does not describe a tree of ncell leaves'
  do iStar = 1, ns
     st(iStar)%level = slev(iStar)
     st(iStar)%weight = 1
     allocate(st(iStar)%position(3*slev(iStar)+3))
     st(iStar)%position = spos(1:3*slev(iStar)+3,iStar)
  enddo

  ! equiSources.f90:1038-1061
  do iStar = 1, ns
     currentStar => st(iStar)
     if (currentStar%weight.gt.0) then
        startingPoint%x = 0.5
        startingPoint%y = 0.5
        startingPoint%z = 0.5
        i = currentStar%position(1)
        j = currentStar%position(2)
        k = currentStar%position(3)
        call localizeCellFromStar(baseGrid%cell(i,j,k),currentStar)
        call computeExpansionParameters(psi*currentStar%hostCell%rho/mh)
        call absoluteCoordinates(currentStar%level,currentStar%position,startingPoint,n,n,n)
        sout(iStar,1) = finalRadius
        sout(iStar,2) = densityCoefficient
        sout(iStar,3) = sourceTotalHydrogenDensity
        sout(iStar,4) = xbase
        sout(iStar,5) = ybase
        sout(iStar,6) = zbase
        do i = 1, n
           do j = 1, n
              do k = 1, n
                 call findExpansion(baseGrid%cell(i,j,k), &
                      (dfloat(i)-0.5)/dfloat(n),(dfloat(j)-0.5)/dfloat(n),(dfloat(k)-0.5)/dfloat(n),n)
              enddo
           enddo
        enddo
     endif
  enddo
  ! :1062-1068
  do i = 1, n
     do j = 1, n
        do k = 1, n
           call applyExpansion(baseGrid%cell(i,j,k))
        enddo
     enddo
  enddo

  cursor = 0
  do i = 1, n
     do j = 1, n
        do k = 1, n
           call harvest(baseGrid%cell(i,j,k))
        enddo
     enddo
  enddo
  open(12, file=trim(outName), access='stream', form='unformatted', status='replace')
  write(12) sout
  write(12) outv
  close(12)

contains

  recursive subroutine growCell(c, level)
    type(zoneType), target :: c
    integer, intent(in) :: level
    integer :: a, b, d
    cursor = cursor + 1
    if (cursor > ncell) stop 'expansion_harness: ran past the end of the level list'
    nullify(c%cell)
    c%level = int(level,1)
    c%rhoCoef = 1.
    if (lev(cursor) == level) then
       c%refined = .false.
       c%rho = f(cursor,1)
       c%HI = f(cursor,2)
       c%HeI = f(cursor,3)
       c%HeII = f(cursor,4)
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
       stop 'expansion_harness: level list is not depth-first'
    endif
  end subroutine growCell

  recursive subroutine harvest(c)
    type(zoneType) :: c
    integer :: a, b, d
    if (c%refined) then
       do a = 1, 2
          do b = 1, 2
             do d = 1, 2
                call harvest(c%cell(a,b,d))
             enddo
          enddo
       enddo
    else
       cursor = cursor + 1
       outv(cursor,1) = c%rhoCoef
       outv(cursor,2) = c%rho
       outv(cursor,3) = c%HI
       outv(cursor,4) = c%HeI
       outv(cursor,5) = c%HeII
    endif
  end subroutine harvest

end program expansion_harness
"""


def build_harness(tmp):
    lines = open(os.path.join(REFERENCE, "equiSources.f90")).read().split("\n")
    lift = lambda a, b: lines[a - 1:b]  # noqa: E731  (sed -n 'a,bp')
    mod = ["module expExtract", "  use definitions", "contains", *lift(2597, 2620), *lift(3011, 3047), *lift(4395, 4503),
           "end module expExtract", ""]
    with open(os.path.join(tmp, "expExtract.f90"), "w") as f:
        f.write("\n".join(mod))
    with open(os.path.join(tmp, "expansion_harness.f90"), "w") as f:
        f.write(DRIVER)
    common = [FC, *FFLAGS, "-w", "-module-dir", tmp, "-I", REF_BUILD]
    subprocess.check_call([*common, "-c", os.path.join(tmp, "expExtract.f90"), "-o", os.path.join(tmp, "expExtract.o")])
    exe = os.path.join(tmp, "expansion_harness")
    subprocess.check_call([*common, os.path.join(tmp, "expansion_harness.f90"), os.path.join(tmp, "expExtract.o"),
                           os.path.join(REF_BUILD, "definitionsModule.o"), "-o", exe])
    return exe


def write_case(path, n, level, box, rho, HI, HeI, HeII, star_level, star_position):
    """the stream file the harness and fortran/ftte_demo_expansion read"""
    with open(path, "wb") as f:
        f.write(struct.pack("<4i", n, len(level), len(star_level), star_position.shape[1]))
        f.write(struct.pack("<d", box))
        f.write(np.asarray(level, "<i4").tobytes())
        for a in (rho, HI, HeI, HeII):
            f.write(np.asarray(a, "<f8").tobytes())
        f.write(np.asarray(star_level, "<i4").tobytes())
        f.write(np.asarray(star_position, "<i4").tobytes())


def run_reference(exe, tmp, n, level, box, rho, HI, HeI, HeII, src_cell):
    ncell, ns = len(level), len(src_cell)
    base, path = X.leaf_paths(n, level)
    maxpos = 3 * (int(np.max(level)) + 1)
    star_level = np.array([len(path[int(c)]) for c in src_cell], np.int32)
    star_position = np.zeros((ns, maxpos), np.int32)
    for s, c in enumerate(src_cell):
        seq = X.call_sequence(base[int(c)], path[int(c)])
        star_position[s, :len(seq)] = seq
    case, out = os.path.join(tmp, "case.bin"), os.path.join(tmp, "out.bin")
    if os.path.exists(out):
        os.remove(out)
    write_case(case, n, level, box, rho, HI, HeI, HeII, star_level, star_position)
    res = subprocess.run([exe, case, out], capture_output=True, text=True)
    if res.returncode != 0 or not os.path.exists(out):
        raise RuntimeError(f"the reference stopped: {res.stdout[-800:]} {res.stderr[-500:]}")
    raw = np.fromfile(out, dtype="<f8")
    assert raw.size == 6 * ns + 5 * ncell
    s = raw[:6 * ns].reshape(6, ns).T      # Fortran (ns,6)
    c = raw[6 * ns:].reshape(5, ncell)     # Fortran (ncell,5)
    return dict(n=n, level=np.asarray(level, np.int32), box=box, rho=rho, HI=HI, HeI=HeI, HeII=HeII,
                src_cell=np.asarray(src_cell, np.int64), star_level=star_level, star_position=star_position,
                params=np.ascontiguousarray(s[:, :3]), centres=np.ascontiguousarray(s[:, 3:]),
                rho_coef=c[0].copy(), rho_out=c[1].copy(), HI_out=c[2].copy(), HeI_out=c[3].copy(), HeII_out=c[4].copy())


def species_of(rng, rho):
    nh = X.PSI * rho / X.MH
    nhe = (1 - X.PSI) * rho / (2 * (X.F32(1.6726231e-24) + X.F32(1.67492728e-24)))
    return nh * 10 ** rng.uniform(-4, 0, rho.size), nhe * rng.uniform(0, 0.7, rho.size), nhe * rng.uniform(0, 0.3, rho.size)


def rho_for(nh, exact):
    """a density whose psi*rho/mh is nh, exactly where that is asked for"""
    rho = nh * X.MH / X.PSI
    if not exact:
        return rho
    for _ in range(64):
        got = X.PSI * rho / X.MH
        if got == nh:
            return rho
        rho = np.nextafter(rho, np.inf if got < nh else -np.inf)
    raise AssertionError(f"no density gives nh = {nh} exactly")


def scattered_levels(n, ones, twos):
    """base cells `ones` refined once, `twos` twice, the rest left alone: the pieces are synthetic.refine_levels' own"""
    piece = {0: np.zeros(1, np.int32), 1: synthetic.refine_levels(1, [(0, 0, 0)], 1), 2: synthetic.refine_levels(1, [(0, 0, 0)], 2)}
    depth = np.zeros(n ** 3, np.int64)
    depth[ones] = 1
    depth[twos] = 2
    return np.concatenate([piece[int(d)] for d in depth]), depth


def check_refined(g):
    """what the first golden has to exercise"""
    n, level, box = g["n"], g["level"], g["box"]
    nh_src = g["params"][:, 2]
    hit = [X.table_interval(v) for v in nh_src]
    assert {i for i, below in hit if not below} == set(range(2, 11)), "every table interval"
    assert any(math.log10(v) in X.LI[1:] for v in nh_src), "a table node exactly"
    assert (nh_src < 1).any() and (nh_src > 1e3).any()
    low = nh_src < 1e-6
    assert low.any() and (g["params"][low, 1] > 1).all(), "below 1e-6 the coefficient exceeds 1"
    assert len(set(g["src_cell"].tolist())) < len(g["src_cell"]), "stars sharing a leaf"
    src_level = level[g["src_cell"]]
    assert (src_level == 0).any() and (src_level == 1).any() and (src_level == 2).any()
    centres = X.leaf_centres(n, level)
    nh = X.PSI * g["rho"] / X.MH
    inside_too_dense = 0
    lowest_from_earlier = 0
    best = np.ones(level.size)
    for (xb, yb, zb), (radius, coef, nhs) in zip(g["centres"], g["params"]):
        d = box * np.sqrt((xb - centres[:, 0]) ** 2 + (yb - centres[:, 1]) ** 2 + (zb - centres[:, 2]) ** 2)
        inside = d < radius
        ok = inside & (nh <= X.MARGIN * nhs)
        inside_too_dense += int((inside & ~ok).sum())
        lowest_from_earlier += int((ok & (best < 1) & (coef > best)).sum())   # a later star's sphere that does not lower rhoCoef
        best[ok] = np.minimum(best[ok], coef)
    assert inside_too_dense > 0 and lowest_from_earlier > 0
    assert np.array_equal(best, g["rho_coef"])
    changed = g["rho_coef"] < 1
    for refined in (False, True):
        sel = (level > 0) == refined
        assert (changed & sel).any() and (~changed & sel).any(), "changed and unchanged leaves in base and in refined cells"
    print(f"expansion_refined: {level.size} leaves, {int(changed.sum())} changed, {inside_too_dense} star-leaf pairs inside a radius "
          f"but too dense, {lowest_from_earlier} where a later star does not lower rhoCoef")


def main():
    if not os.path.exists(os.path.join(REF_BUILD, "definitionsModule.o")):
        sys.exit("build the reference's modules first: make -C oracle ref")
    tmp = tempfile.mkdtemp()
    try:
        exe = build_harness(tmp)
        # (1) refined, 12^3 base
        rng = np.random.default_rng(1035)
        n, box = 12, 3.0 * KPC
        cells = rng.permutation(n ** 3)
        level, depth = scattered_levels(n, cells[:60], cells[60:100])
        rho = 10 ** rng.uniform(-3, 3.5, level.size) * X.MH / X.PSI
        first = np.concatenate([[0], np.cumsum(8 ** depth)[:-1]])        # first leaf of every base cell
        hosts = np.concatenate([first[cells[100:220]],                    # base leaves
                                first[cells[:60]] + rng.integers(0, 8, 60),      # level 1
                                first[cells[60:100]] + rng.integers(0, 64, 40)])  # level 2
        src = np.concatenate([hosts, rng.choice(hosts, 80)])              # 300 stars, 80 of them in a leaf that has one already
        special = [1e-7, 5e-7, 1e-3, 0.5, 1.0, 10.0, 1000.0, 5e4, 2.0e3] + [10 ** (0.1667 + k / 3.0) for k in range(9)]
        for cell, v in zip(hosts[::9], special):
            rho[cell] = rho_for(v, v in (1.0, 10.0, 1000.0))
        HI, HeI, HeII = species_of(rng, rho)
        g = run_reference(exe, tmp, n, level, box, rho, HI, HeI, HeII, src)
        check_refined(g)
        save("expansion_refined", g)
        # (2) uniform 16^3
        rng = np.random.default_rng(1036)
        n, box = 16, 4.0 * KPC
        level = np.zeros(n ** 3, np.int32)
        rho = 10 ** rng.uniform(-2, 3, level.size) * X.MH / X.PSI
        HI, HeI, HeII = species_of(rng, rho)
        g = run_reference(exe, tmp, n, level, box, rho, HI, HeI, HeII, rng.choice(n ** 3, 40))
        assert 0 < (g["rho_coef"] < 1).sum() < level.size
        save("expansion_uniform16", g)
        # (3) the tree the reference's ingest built
        rng = np.random.default_rng(1037)
        src_g = np.load(os.path.join(HERE, "ingest6_three_levels_metals_velocities.npz"))
        n, level, box = int(src_g["out_n"]), src_g["out_level"].astype(np.int32), 60.0 * KPC
        rho, HI, HeI, HeII = (src_g["out_" + k].astype(np.float64) for k in ("rho", "HI", "HeI", "HeII"))
        stars = np.sort(rng.choice(level.size, 12, replace=False))
        g = run_reference(exe, tmp, n, level, box, rho, HI, HeI, HeII, stars)
        assert 0 < (g["rho_coef"] < 1).sum() < level.size
        save("expansion_ingested", g)
    finally:
        shutil.rmtree(tmp)


if __name__ == "__main__":
    main()
