#!/usr/bin/env python3
"""Golden vectors for the analysis modes, produced by the reference's own compiled lines: the slice map of its reader
(readCellArray.f90:116-140, sliceCell :189-230), the projection of mode initialConfiguration (equiSources.f90:685-719,
projectVariableToMap :4914-4954), the clumping factor (:662-674, computeClumping :4711-4735) and the gas PDF (:814-822,
computeGasPDF :4682-4709).

    python -m radiativetransfer_amd.build && make -C oracle && make -C oracle ref && python tests/golden/make_golden_analysis.py

oracle/ stays as it is: as make_golden_initial.py does, this script lifts the routines and the pixel loops by line range into a
module, wraps the loops into subroutines that carry the main programs' own declarations (equiSources.f90:27-44, :69-75;
readCellArray.f90:6-11, :14), writes a small driver program next to it, and compiles both with the oracle's compiler and flags
against the definitionsModule and rotateIndicesModule objects that `make -C oracle ref` leaves in oracle/_ref/ -- all in a temporary
directory that is deleted afterwards.  Only the .npz files (data) are written into the tree:

  analysis_refined6.npz    the tree of amr6_scattered_level2.npz (6^3 base, two levels), a log-normal rho with a column of rho = 0
                           and cells below and above the PDF's range, abun2 and HI uncorrelated with it; all 24 izones
  analysis_ingested12.npz  the three-level grid the reference's ingest built (ingest6_three_levels_metals_velocities.npz)
  analysis_uniform16.npz   a uniform 16^3 grid
  analysis_uniform12.npz   a uniform 12^3 grid

Each holds the medium, a job table (kind 1 slice, 2 projection; izone; map size; zslice or centre and zoom) and per job the map
with the per-column and per-row quantities i0, xnew, j0, ynew and k0, znew or kstart, kend, then the clumping sums with the printed
ratio and pdfGas, pdfGasOutside.  The generator asserts that no leaf's log10(rho/msun*pc**3) lies within 8 ulp of a bin edge or of
the range's ends (a device log10 may differ from the host's in the last bit) and takes another seed where one does.  The files are
written with fixed zip timestamps, so a rerun reproduces them byte for byte.
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
REF_BUILD = os.path.join(ROOT, "oracle", "_ref")
REFERENCE = os.environ.get("REFERENCE", "/root/reference")
FC = shutil.which("amdflang") or "/opt/rocm/bin/amdflang"
FFLAGS = os.environ.get("FFLAGS", "-O2").split()

sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
from make_golden_initial import save  # noqa: E402
import _analysis as A  # noqa: E402

# what the wrappers hand over, beside the reference's own module variables
STATE = """
  integer :: axN, axIzone, axNxmap, axNymap
  real(kind=RealKind) :: axCentre(3), axZoom, axSlice, axZnew, axRaw(3), axRatio
  integer :: axK(2)
  real*4, dimension(:,:), pointer :: axMap
  integer, allocatable :: axI0(:), axJ0(:)
  real(kind=RealKind), allocatable :: axX(:), axY(:)
"""

DRIVER = r"""
! the analysis modes on a cell array handed over in a stream file (generated; see make_golden_analysis.py)
! case: int32 n, ncell ; real64 box ; int32 level(ncell) ; real64 f(ncell,3) = rho, abun2, HI ; int32 njobs ;
!       per job int32 kind, izone, nxmap, nymap ; real64 p(4) = zslice | centre(3), zoom
! out:  per job real32 map(nxmap,nymap) ; int32 i0(nxmap) ; real64 xnew(nxmap) ; int32 j0(nymap) ; real64 ynew(nymap) ;
!       int32 k(2) ; real64 znew ; then real64 raw sums (3), ratio ; real64 pdfGas(npdf), pdfGasOutside
program analysis_harness
  use definitions
  use analysisExtract
  implicit none
  integer :: n, ncell, cursor, bi, bj, bk, njobs, q, jobKind
  integer, allocatable :: lev(:)
  real(kind=RealKind), allocatable :: f(:,:)
  real(kind=RealKind) :: box, p(4)
  character(len=512) :: caseName, outName

  call get_command_argument(1, caseName)
  call get_command_argument(2, outName)
  open(11, file=trim(caseName), access='stream', form='unformatted', status='old')
  read(11) n, ncell
  read(11) box
  allocate(lev(ncell), f(ncell,3))
  read(11) lev
  read(11) f
  physicalBoxSize = box
  axN = n

  baseGrid%refined = .true.
  baseGrid%level = -1
  allocate(baseGrid%cell(n,n,n))
  cursor = 0
  do bi = 1, n
     do bj = 1, n
        do bk = 1, n
           baseGrid%cell(bi,bj,bk)%parent => baseGrid
           call growCell(baseGrid%cell(bi,bj,bk), 0)
        enddo
     enddo
  enddo
  if (cursor /= ncell) stop 'analysis_harness: level list does not describe a tree of ncell leaves'

  open(12, file=trim(outName), access='stream', form='unformatted', status='replace')
  read(11) njobs
  do q = 1, njobs
     read(11) jobKind, axIzone, axNxmap, axNymap
     read(11) p
     if (jobKind == 1) then
        axSlice = p(1)
        call referenceSlice()
     else
        axCentre = p(1:3)
        axZoom = p(4)
        axZnew = 0.
        call referenceProject()
     endif
     write(12) axMap
     write(12) axI0, axX, axJ0, axY, axK, axZnew
     deallocate(axMap, axI0, axX, axJ0, axY)
  enddo
  close(11)
  call referenceClumping()
  write(12) axRaw, axRatio
  call referenceGasPDF()
  write(12) pdfGas, pdfGasOutside
  close(12)

contains

  recursive subroutine growCell(c, level)
    type(zoneType), target :: c
    integer, intent(in) :: level
    integer :: a, b, d
    cursor = cursor + 1
    if (cursor > ncell) stop 'analysis_harness: ran past the end of the level list'
    nullify(c%cell)
    c%level = int(level,1)
    if (lev(cursor) == level) then
       c%refined = .false.
       c%rho = f(cursor,1)
       c%abun2 = f(cursor,2)
       c%HI = f(cursor,3)
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
       stop 'analysis_harness: level list is not depth-first'
    endif
  end subroutine growCell

end program analysis_harness
"""


def build_harness(tmp):
    eq = open(os.path.join(REFERENCE, "equiSources.f90")).read().split("\n")
    rd = open(os.path.join(REFERENCE, "readCellArray.f90")).read().split("\n")
    E = lambda a, b=None: eq[a - 1:(b or a)]  # noqa: E731  (sed -n 'a,bp')
    R = lambda a, b=None: rd[a - 1:(b or a)]  # noqa: E731
    size = ["    nx = axN", "    ny = axN", "    nz = axN"]
    tables = lambda col, row: [  # noqa: E731  the per-column and per-row lines of a pixel loop once more, their results kept
        "    allocate(axI0(nxmap), axX(nxmap), axJ0(nymap), axY(nymap))",
        "    do i = 1, nxmap", *col, "       axI0(i) = i0", "       axX(i) = xnew", "    enddo",
        "    do j = 1, nymap", *row, "       axJ0(j) = j0", "       axY(j) = ynew", "    enddo"]
    mod = ["module analysisExtract", "  use definitions", "  use rotateIndicesModule", STATE, "contains",
           *E(4682, 4735), *E(4914, 4954), *R(189, 230),
           "  subroutine referenceProject()", *E(27, 44), *E(69, 75),
           "    izone = int(axIzone,1)", "    nxmap = axNxmap", "    nymap = axNymap", "    centerPoint = axCentre", "    zoomFactor = axZoom", *size,
           *E(685, 719),
           "    axMap => mapArray", "    axK(1) = kstart", "    axK(2) = kend",
           *tables([*E(703, 704), *E(708)], [*E(706, 707), *E(709)]),
           "  end subroutine referenceProject",
           "  subroutine referenceSlice()", *R(6, 11), *R(14),
           "    izone = int(axIzone,1)", "    nxmap = axNxmap", "    nymap = axNymap", "    zslice = axSlice", *size,
           *R(116, 140),
           "    axMap => mapArray", "    axK(1) = k0", "    axK(2) = k0", "    axZnew = znew",
           *tables([*R(126, 127), *R(131)], [*R(129, 130), *R(132)]),
           "  end subroutine referenceSlice",
           "  subroutine referenceClumping()", *E(27, 44), *size,
           *E(662, 671),
           "    axRaw(1) = volSum", "    axRaw(2) = volSumDensity", "    axRaw(3) = volSumDensity2",
           *E(672, 673),
           "    axRatio = volSumDensity2 / volSumDensity**2",
           "  end subroutine referenceClumping",
           "  subroutine referenceGasPDF()", *E(27, 44), *size,
           *E(814, 822),
           "  end subroutine referenceGasPDF",
           "end module analysisExtract", ""]
    with open(os.path.join(tmp, "analysisExtract.f90"), "w") as f:
        f.write("\n".join(mod))
    with open(os.path.join(tmp, "analysis_harness.f90"), "w") as f:
        f.write(DRIVER)
    common = [FC, *FFLAGS, "-w", "-module-dir", tmp, "-I", REF_BUILD]
    subprocess.check_call([*common, "-c", os.path.join(tmp, "analysisExtract.f90"), "-o", os.path.join(tmp, "analysisExtract.o")])
    exe = os.path.join(tmp, "analysis_harness")
    subprocess.check_call([*common, os.path.join(tmp, "analysis_harness.f90"), os.path.join(tmp, "analysisExtract.o"),
                           os.path.join(REF_BUILD, "definitionsModule.o"), os.path.join(REF_BUILD, "rotateIndicesModule.o"), "-o", exe])
    return exe


def run_reference(exe, tmp, n, level, box, rho, abun2, HI, jobs):
    ncell = len(level)
    case, out = os.path.join(tmp, "case.bin"), os.path.join(tmp, "out.bin")
    if os.path.exists(out):
        os.remove(out)
    with open(case, "wb") as f:
        f.write(struct.pack("<2i", n, ncell))
        f.write(struct.pack("<d", box))
        f.write(np.asarray(level, "<i4").tobytes())
        for a in (rho, abun2, HI):
            f.write(np.asarray(a, "<f8").tobytes())
        f.write(struct.pack("<i", len(jobs)))
        for kind, izone, nx, ny, p in jobs:
            f.write(struct.pack("<4i", kind, izone, nx, ny))
            f.write(struct.pack("<4d", *p))
    res = subprocess.run([exe, case, out], stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, text=True)  # (the loops print every column)
    if res.returncode != 0 or not os.path.exists(out):
        raise RuntimeError(f"the reference stopped: {res.stderr[-800:]}")
    raw = open(out, "rb").read()
    at = 0

    def take(dtype, count):
        nonlocal at
        a = np.frombuffer(raw, dtype=dtype, count=count, offset=at).copy()
        at += a.nbytes
        return a

    o = {}
    for q, (kind, izone, nx, ny, p) in enumerate(jobs):
        o[f"job{q}_map"] = take("<f4", nx * ny).reshape(ny, nx).T  # mapArray(nxmap,nymap) -> [nxmap][nymap]
        o[f"job{q}_i0"], o[f"job{q}_xnew"] = take("<i4", nx), take("<f8", nx)
        o[f"job{q}_j0"], o[f"job{q}_ynew"] = take("<i4", ny), take("<f8", ny)
        o[f"job{q}_k"], o[f"job{q}_znew"] = take("<i4", 2), take("<f8", 1)[0]
    sums = take("<f8", 4)
    o.update(volSum=sums[0], volSumDensity=sums[1], volSumDensity2=sums[2], clumping=sums[3])
    o["pdfGas"], o["pdfGasOutside"] = take("<f8", A.NPDF), take("<f8", 1)[0]
    assert at == len(raw)
    o["jobs_kind"] = np.array([j[0] for j in jobs], dtype=np.int32)
    o["jobs_izone"] = np.array([j[1] for j in jobs], dtype=np.int32)
    o["jobs_shape"] = np.array([j[2:4] for j in jobs], dtype=np.int32)
    o["jobs_p"] = np.array([j[4] for j in jobs], dtype=np.float64)
    return o


def pdf_is_safe(rho):
    """no leaf within 8 ulp of a place where its bin, or inside / outside, changes"""
    tmp = A.pdf_log(rho)
    finite = np.isfinite(tmp)
    lo, hi = tmp.copy(), tmp.copy()
    for _ in range(8):
        lo[finite], hi[finite] = np.nextafter(lo[finite], -np.inf), np.nextafter(hi[finite], np.inf)
    bins = A.pdf_bins(tmp)
    return bool(np.all(A.pdf_bins(lo) == bins) and np.all(A.pdf_bins(hi) == bins))


def synthetic_medium(seed, tree, zero_column=True):
    """a log-normal rho around 1e-3 msun/pc^3 with cells below and above the PDF's range and rho = 0; abun2, HI on their own"""
    unit = A.MSUN / A.PC ** 3
    while True:
        rng = np.random.default_rng(seed)
        ncell = tree.ncell
        rho = unit * 10.0 ** rng.normal(-3.0, 1.5, ncell)
        rho[3::41] = unit * 10.0 ** rng.uniform(-11.0, -8.5, rho[3::41].size)  # below apdf
        rho[5::53] = unit * 10.0 ** rng.uniform(3.2, 5.0, rho[5::53].size)     # above bpdf
        if zero_column:
            n = tree.n
            rho[(tree.base_of_leaf // n) == (1 * n + 2)] = 0.0  # every leaf of the base cells (icell, jcell) = (2, 3)
        abun2 = 0.02 * 10.0 ** rng.normal(0.0, 0.5, ncell)
        HI = 10.0 ** rng.uniform(-9.0, 1.0, ncell)
        if pdf_is_safe(rho):
            return rho, abun2, HI
        seed += 1


def standard_jobs(n, izones=(2, 3)):
    """the slices and projections every refined case gets"""
    jobs = []
    for shape in ((50, 37), (7, 5), (200, 3)):
        for zslice in (0.0, 0.5, 0.6180339887498949, 0.999):  # 0.5 lies exactly on a base-cell boundary of n = 6 and 12
            jobs.append((1, izones[0], *shape, (zslice, 0.0, 0.0, 0.0)))
        for centre, zoom in (((0.5, 0.5, 0.5), 1.0), ((0.5, 0.5, 0.5), 2.0), ((0.1, 0.93, 0.9), 3.0)):
            jobs.append((2, izones[1], *shape, (*centre, zoom)))
    return jobs


def main():
    for mod in ("definitionsModule.o", "rotateIndicesModule.o"):
        if not os.path.exists(os.path.join(REF_BUILD, mod)):
            sys.exit("build the reference's modules first: make -C oracle ref")
    tmp = tempfile.mkdtemp()
    try:
        exe = build_harness(tmp)
        # (a) the scattered two-level tree, all 24 izones
        amr = np.load(os.path.join(HERE, "amr6_scattered_level2.npz"))
        n, level, box = int(amr["n"]), amr["level"].astype(np.int32), 2.5e23
        rho, abun2, HI = synthetic_medium(661, A.Tree(n, level))
        jobs = standard_jobs(n)
        for izone in range(1, 25):
            jobs.append((1, izone, 13, 11, (0.31, 0.0, 0.0, 0.0)))
            jobs.append((2, izone, 13, 11, (0.5, 0.5, 0.5, 1.0)))
        o = run_reference(exe, tmp, n, level, box, rho, abun2, HI, jobs)
        assert np.isnan(o[f"job{len(standard_jobs(n)) + 1}_map"]).any(), "izone 1 projects through the column of rho = 0"
        save("analysis_refined6", dict(n=n, level=level, box=box, rho=rho, abun2=abun2, HI=HI, **o))
        # (b) the grid the reference's ingest built
        g = np.load(os.path.join(HERE, "ingest6_three_levels_metals_velocities.npz"))
        n, level, box = int(g["out_n"]), g["out_level"].astype(np.int32), float(g["out_box"])
        rho, abun2, HI = (g["out_" + k].astype(np.float64) for k in ("rho", "abun2", "HI"))
        assert pdf_is_safe(rho)
        o = run_reference(exe, tmp, n, level, box, rho, abun2, HI, standard_jobs(n, izones=(17, 8)))
        save("analysis_ingested12", dict(n=n, level=level, box=box, rho=rho, abun2=abun2, HI=HI, **o))
        # (c) a uniform grid
        n, box = 16, 3.0e24
        level = np.zeros(n ** 3, dtype=np.int32)
        rho, abun2, HI = synthetic_medium(785, A.Tree(n, level), zero_column=False)
        jobs = [(1, 2, 50, 37, (0.506896972656250, 0.0, 0.0, 0.0)), (1, 11, 7, 5, (0.0, 0.0, 0.0, 0.0)),
                (2, 3, 50, 37, (0.5, 0.5, 0.5, 2.0)), (2, 22, 200, 3, (0.1, 0.93, 0.9, 3.0)), (2, 6, 7, 5, (0.5, 0.5, 0.5, 1.0))]
        o = run_reference(exe, tmp, n, level, box, rho, abun2, HI, jobs)
        save("analysis_uniform16", dict(n=n, level=level, box=box, rho=rho, abun2=abun2, HI=HI, **o))
        # (d) a uniform 12^3 grid under every window and map size of the refined cases: the axis tables of a third base grid size
        n, box = 12, 1.0e24
        level = np.zeros(n ** 3, dtype=np.int32)
        rho, abun2, HI = synthetic_medium(814, A.Tree(n, level), zero_column=False)
        o = run_reference(exe, tmp, n, level, box, rho, abun2, HI, standard_jobs(n, izones=(5, 24)))
        save("analysis_uniform12", dict(n=n, level=level, box=box, rho=rho, abun2=abun2, HI=HI, **o))
    finally:
        shutil.rmtree(tmp)


if __name__ == "__main__":
    main()
