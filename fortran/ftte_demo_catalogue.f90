! ftte_demo_catalogue.f90 -- a Fortran host for the star catalogue in the shape of the reference's blocks equiSources.f90:746-769,
! :1169-1212 and :1282-1293, through ftte_binding, without the reference's modules: the stars come as coordinates in the units of the
! box corners, their host leaves, the merged sources and the sources' metallicity brackets come back.
!
!   ftte_demo_catalogue <case.bin> <out.bin>
!
! case.bin (stream): int32 n, ncell, nstars ; real64 lo(3), hi(3) ; int32 level(ncell) ; real64 abun2(ncell) ; real64 xyz(3,nstars) ;
!   int32 weight(nstars) ; real64 metallicity(5)
! out.bin: int64 nsrc, outside ; int64 starCell(nstars) ; int32 starLevel(nstars), starPosition(33,nstars) (zero-padded) ;
!   int64 srcCell(nsrc), srcFirstStar(nsrc) ; int32 srcWeight(nsrc), iMetal(nsrc), srcSlot(nsrc) ;
!   real64 srcNdot(nsrc), srcAbun2(nsrc), coefMetal(nsrc)
program ftte_demo_catalogue

  use, intrinsic :: iso_c_binding
  use ftte_binding
  implicit none

  integer, parameter :: maxpos = 33
  integer(c_int32_t) :: n, ncell32, ns
  integer(c_int64_t) :: ncell, nsrc, outside, npop
  type(c_ptr) :: ctx
  integer(c_int32_t), allocatable, target :: lev(:), w(:), slev(:), spos(:,:), srcWeight(:), iMetal(:), srcSlot(:)
  integer(c_int64_t), allocatable, target :: starCell(:), srcCell(:), srcFirst(:), popFirst(:)
  real(c_double), allocatable, target :: ab(:), xyz(:,:), srcNdot(:), srcAbun2(:), coefMetal(:)
  real(c_double) :: lo(3), hi(3), metallicity(5)
  integer(c_int32_t) :: pos(183)
  integer(c_int) :: level
  character(len=512) :: caseName, outName
  integer :: ios, iStar

  call get_command_argument(1, caseName)
  call get_command_argument(2, outName)
  open(11, file=trim(caseName), access='stream', form='unformatted', status='old', iostat=ios)
  if (ios /= 0) stop 'ftte_demo_catalogue: cannot open case file'
  read(11) n, ncell32, ns
  read(11) lo, hi
  ncell = ncell32
  allocate(lev(ncell), ab(ncell), xyz(3,ns), w(ns), starCell(ns), slev(ns), spos(maxpos,ns))
  read(11) lev
  read(11) ab
  read(11) xyz
  read(11) w
  read(11) metallicity
  close(11)

  call ftteCheck(c_null_ptr, ftte_create(ctx, 1, c_null_ptr), 'ftte_create')
  call ftteCheck(ctx, ftte_set_grid(ctx, n, n, n, ncell, lev, 1.0d0), 'ftte_set_grid')
  ! (only abun2 is read here; it stands in for the other fields)
  call ftteCheck(ctx, ftte_set_medium(ctx, ab, ab, ab, ab, ab, 0), 'ftte_set_medium')
  call ftteCheck(ctx, ftte_star_catalogue(ctx, int(ns, c_int64_t), xyz, lo, hi, c_loc(w), c_loc(starCell), nsrc, outside), &
       'ftte_star_catalogue')
  allocate(srcCell(nsrc), srcFirst(nsrc), srcWeight(nsrc), iMetal(nsrc), srcSlot(nsrc), srcNdot(nsrc), srcAbun2(nsrc), &
       coefMetal(nsrc), popFirst(max(nsrc,1_c_int64_t)))
  call ftteCheck(ctx, ftte_star_sources(ctx, nsrc, c_loc(srcCell), c_loc(srcWeight), c_loc(srcNdot), c_loc(srcFirst), &
       c_loc(srcAbun2)), 'ftte_star_sources')
  call ftteCheck(c_null_ptr, ftte_star_populations(5, metallicity, nsrc, srcAbun2, iMetal, coefMetal, srcSlot, npop, popFirst), &
       'ftte_star_populations')
  spos = 0
  slev = -1
  do iStar = 1, ns
     if (starCell(iStar) .ge. 0) then
        call ftteCheck(ctx, ftte_cell_position(ctx, starCell(iStar), level, pos), 'ftte_cell_position')
        slev(iStar) = level
        spos(1:3*level+3,iStar) = pos(1:3*level+3)
     endif
  enddo

  open(12, file=trim(outName), access='stream', form='unformatted', status='replace')
  write(12) nsrc, outside
  write(12) starCell
  write(12) slev, spos
  write(12) srcCell, srcFirst
  write(12) srcWeight, iMetal, srcSlot
  write(12) srcNdot, srcAbun2, coefMetal
  close(12)
  write(*,'(a,i4,a,i9,a,i9,a,i9,a,i9,a,i9)') ' grid ', n, '^3 base, ', ncell, ' cells, ', ns, ' stars, ', nsrc, ' sources, ', &
       outside, ' outside, populations ', npop
  write(*,*) 'ftte_demo_catalogue OK'
  call ftteCheck(ctx, ftte_destroy(ctx), 'ftte_destroy')

end program ftte_demo_catalogue
