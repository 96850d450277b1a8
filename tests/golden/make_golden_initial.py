#!/usr/bin/env python3
"""Golden vectors for the start-up ionisation equilibrium (equiSources.f90:1008-1022): initialIonizationEquilibrium
(:3679-3868) twice per leaf, then computeMass (:4369-4393), produced by the reference's own compiled lines.

    python -m radiativetransfer_amd.build && make -C oracle && make -C oracle ref && python tests/golden/make_golden_initial.py

oracle/ stays as it is: this script lifts the two routines and `opposite` (:5044-5058) by line range into a module, the way
oracle/Makefile lifts chemExtract, writes a small driver program next to it, and compiles both with the oracle's compiler and
flags against the definitionsModule object that `make -C oracle ref` leaves in oracle/_ref/ -- all in a temporary directory
that is deleted afterwards.  Only the .npz files (data) are written into the tree:

  initial_refined.npz   (a) a refined synthetic cell array (make_golden_chem.synthetic_gas; the rate-coefficient tables of
                            chem_uvb_refined.npz): temperatures below and above the table, HI > nh, both branches of the
                            HeIII clip, lit and self-shielded cells
  initial_ingested.npz  (b) the start-up on the grid the reference's ingest built (ingest6_three_levels_metals_velocities.npz)

Each holds the inputs, HI_out, HeI_out, HeII_out after both passes and the reference's sequential sums neutral_mass,
total_mass [msun].  The files are written with fixed zip timestamps, so a rerun reproduces them byte for byte.
"""
import io
import os
import shutil
import struct
import subprocess
import sys
import tempfile
import zipfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF_BUILD = os.path.join(ROOT, "oracle", "_ref")
REFERENCE = os.environ.get("REFERENCE", "/root/reference")
FC = shutil.which("amdflang") or "/opt/rocm/bin/amdflang"
FFLAGS = os.environ.get("FFLAGS", "-O2").split()
NRATEC = 5000

sys.path.insert(0, HERE)
from make_golden_chem import synthetic_gas  # noqa: E402

DRIVER = r"""
! the start-up of equiSources.f90:1008-1022 on a cell array handed over in a stream file (generated; see make_golden_initial.py)
! case: int32 n, ncell ; real64 box ; int32 level(ncell) ; real64 f(ncell,5) = rho, tgas, HI, HeI, HeII ; real64 uniform(3) ;
!       real64 selfShieldingThreshold ; real64 logtem0, logtem9, dlogtem ; real64 k1a..k6a (nratec each)
! out:  real64 neutralHydrogenMass, totalHydrogenMass ; real64 HI, HeI, HeII (ncell each)
program initial_harness
  use definitions
  use initExtract
  implicit none
  integer :: n, ncell, cursor, bi, bj, bk, ilambda
  integer, allocatable :: lev(:)
  real(kind=RealKind), allocatable :: f(:,:), outv(:,:)
  real(kind=RealKind) :: box, uni(3)
  character(len=512) :: caseName, outName

  call get_command_argument(1, caseName)
  call get_command_argument(2, outName)
  open(11, file=trim(caseName), access='stream', form='unformatted', status='old')
  read(11) n, ncell
  read(11) box
  allocate(lev(ncell), f(ncell,5), outv(ncell,3))
  read(11) lev
  read(11) f
  read(11) uni
  read(11) selfShieldingThreshold
  read(11) logtem0, logtem9, dlogtem
  read(11) k1a, k2a, k3a, k4a, k5a, k6a
  close(11)
  physicalBoxSize = box
  uniformQuasar = 1.
  uniformStellar = 0.
  quasar%ksi24 = uni(1) ; quasar%ksi25 = uni(2) ; quasar%ksi26 = uni(3)
  stellar%ksi24 = 0. ; stellar%ksi25 = 0. ; stellar%ksi26 = 0.

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
  if (cursor /= ncell) stop 'initial_harness: level list does not describe a tree of ncell leaves'

  ncosmic = ncell
  neutralHydrogenMass = 0.
  totalHydrogenMass = 0.
  icosmic = 0
  do bi = 1, n
     do bj = 1, n
        do bk = 1, n
           do ilambda = 1, 2
              call initialIonizationEquilibrium(baseGrid%cell(bi,bj,bk))
           enddo
           call computeMass(baseGrid%cell(bi,bj,bk),n)
        enddo
     enddo
  enddo

  cursor = 0
  do bi = 1, n
     do bj = 1, n
        do bk = 1, n
           call harvest(baseGrid%cell(bi,bj,bk))
        enddo
     enddo
  enddo
  open(12, file=trim(outName), access='stream', form='unformatted', status='replace')
  write(12) neutralHydrogenMass, totalHydrogenMass
  write(12) outv
  close(12)

contains

  recursive subroutine growCell(c, level)
    type(zoneType), target :: c
    integer, intent(in) :: level
    integer :: a, b, d
    cursor = cursor + 1
    if (cursor > ncell) stop 'initial_harness: ran past the end of the level list'
    nullify(c%cell)
    c%level = int(level,1)
    if (lev(cursor) == level) then
       c%refined = .false.
       c%rho = f(cursor,1)
       c%tgas = f(cursor,2)
       c%HI = f(cursor,3)
       c%HeI = f(cursor,4)
       c%HeII = f(cursor,5)
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
       stop 'initial_harness: level list is not depth-first'
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
       outv(cursor,1) = c%HI
       outv(cursor,2) = c%HeI
       outv(cursor,3) = c%HeII
    endif
  end subroutine harvest

end program initial_harness
"""


def build_harness(tmp):
    src = os.path.join(REFERENCE, "equiSources.f90")
    lines = open(src).read().split("\n")
    lift = lambda a, b: lines[a - 1:b]  # noqa: E731  (sed -n 'a,bp')
    mod = ["module initExtract", "  use definitions", "contains", *lift(3679, 3868), *lift(4369, 4393), *lift(5044, 5058),
           "end module initExtract", ""]
    with open(os.path.join(tmp, "initExtract.f90"), "w") as f:
        f.write("\n".join(mod))
    with open(os.path.join(tmp, "initial_harness.f90"), "w") as f:
        f.write(DRIVER)
    common = [FC, *FFLAGS, "-w", "-module-dir", tmp, "-I", REF_BUILD]
    subprocess.check_call([*common, "-c", os.path.join(tmp, "initExtract.f90"), "-o", os.path.join(tmp, "initExtract.o")])
    exe = os.path.join(tmp, "initial_harness")
    subprocess.check_call([*common, os.path.join(tmp, "initial_harness.f90"), os.path.join(tmp, "initExtract.o"),
                           os.path.join(REF_BUILD, "definitionsModule.o"), "-o", exe])
    return exe


def run_reference(exe, tmp, n, level, box, rho, tgas, HI, HeI, HeII, uniform, threshold, tables):
    ncell = len(level)
    case, out = os.path.join(tmp, "case.bin"), os.path.join(tmp, "out.bin")
    if os.path.exists(out):
        os.remove(out)
    with open(case, "wb") as f:
        f.write(struct.pack("<2i", n, ncell))
        f.write(struct.pack("<d", box))
        f.write(np.asarray(level, "<i4").tobytes())
        for a in (rho, tgas, HI, HeI, HeII):
            f.write(np.asarray(a, "<f8").tobytes())
        f.write(np.asarray(uniform, "<f8").tobytes())
        f.write(struct.pack("<d", threshold))
        f.write(struct.pack("<3d", tables["logtem0"], tables["logtem9"], tables["dlogtem"]))
        f.write(np.asarray(tables["k"], "<f8").reshape(6, NRATEC).tobytes())
    res = subprocess.run([exe, case, out], capture_output=True, text=True)
    if res.returncode != 0 or not os.path.exists(out):
        raise RuntimeError(f"the reference stopped: {res.stdout[-800:]} {res.stderr[-500:]}")
    raw = np.fromfile(out, dtype="<f8")
    assert raw.size == 2 + 3 * ncell
    rest = raw[2:]
    return dict(neutral_mass=raw[0], total_mass=raw[1], HI_out=rest[:ncell].copy(), HeI_out=rest[ncell:2 * ncell].copy(),
                HeII_out=rest[2 * ncell:].copy())


def median_mfp(rho, HI, HeI, HeII):
    """a threshold that leaves about half of the cells lit and half self-shielded (first pass)"""
    nh = float(np.float32(0.76)) * rho / float(np.float32(1.6726231e-24))
    mfp = 1.0 / (np.minimum(HI, nh) * float(np.float32(6.3e-18)) + HeI * float(np.float32(7.42e-18)) + HeII * float(np.float32(1.58e-18)))
    return float(np.median(mfp))


def save(name, arrays):
    """np.savez_compressed with fixed timestamps: the same arrays give the same bytes"""
    path = os.path.join(HERE, name + ".npz")
    with zipfile.ZipFile(path, "w", compression=zipfile.ZIP_DEFLATED) as z:
        for key in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(arrays[key]), allow_pickle=False)
            info = zipfile.ZipInfo(key + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            z.writestr(info, buf.getvalue())
    print(f"{name}: {os.path.getsize(path) / 1024:.0f} KiB")


def main():
    if not os.path.exists(os.path.join(REF_BUILD, "definitionsModule.o")):
        sys.exit("build the reference's modules first: make -C oracle ref")
    chem = np.load(os.path.join(HERE, "chem_uvb_refined.npz"))
    tables = {k: chem[k] for k in ("logtem0", "logtem9", "dlogtem", "k")}
    uniform = np.array([3.0e-14, 1.0e-16, 2.0e-14])
    tmp = tempfile.mkdtemp()
    try:
        exe = build_harness(tmp)
        # (a) refined synthetic gas
        rng = np.random.default_rng(1008)
        amr = np.load(os.path.join(HERE, "amr6_scattered_level2.npz"))
        n, level, box = int(amr["n"]), amr["level"].astype(np.int32), 2.5e23
        rho, tgas, HI, HeI, HeII, _, _ = synthetic_gas(rng, level, n, box)
        nhe = (1 - float(np.float32(0.76))) * rho / (2 * (float(np.float32(1.6726231e-24)) + float(np.float32(1.67492728e-24))))
        HeI[7::31] = nhe[7::31] * 1.2      # HeI > nhe: the inner branch of the HeIII clip (HeII = 0)
        HeII[7::31] = nhe[7::31] * 0.1
        threshold = median_mfp(rho, HI, HeI, HeII)
        o = run_reference(exe, tmp, n, level, box, rho, tgas, HI, HeI, HeII, uniform, threshold, tables)
        save("initial_refined", dict(n=n, level=level, box=box, rho=rho, tgas=tgas, HI=HI, HeI=HeI, HeII=HeII, uniform=uniform,
                                     threshold=threshold, **o))
        # (b) the grid the reference's ingest built
        g = np.load(os.path.join(HERE, "ingest6_three_levels_metals_velocities.npz"))
        n, level, box = int(g["out_n"]), g["out_level"].astype(np.int32), float(g["out_box"])
        rho, tgas, HI, HeI, HeII = (g["out_" + k].astype(np.float64) for k in ("rho", "tgas", "HI", "HeI", "HeII"))
        threshold = median_mfp(rho, HI, HeI, HeII)
        o = run_reference(exe, tmp, n, level, box, rho, tgas, HI, HeI, HeII, uniform, threshold, tables)
        save("initial_ingested", dict(n=n, level=level, box=box, rho=rho, tgas=tgas, HI=HI, HeI=HeI, HeII=HeII, uniform=uniform,
                                      threshold=threshold, **o))
    finally:
        shutil.rmtree(tmp)


if __name__ == "__main__":
    main()
