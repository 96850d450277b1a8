! ftte_demo_expansion.f90 -- a Fortran host for the start-up expansion of HII regions in the shape of the reference's block
! equiSources.f90:1035-1069, through ftte_binding, without the reference's modules: the stars come as the reference holds them
! (level + call sequence), their host leaves from ftte_locate_cell, the parameters from the host leaves' densities.
!
!   ftte_demo_expansion <case.bin> <out.bin>
!
! case.bin (stream): int32 n, ncell, nstars, maxpos ; real64 box ; int32 level(ncell) ; real64 rho, HI, HeI, HeII (ncell each) ;
!   int32 starLevel(nstars) ; int32 starPosition(maxpos,nstars)  (base indices 1..n, then child indices 1..2 per level)
! out.bin: real64 rhoCoef, rho, HI, HeI, HeII (ncell each)
program ftte_demo_expansion

  use, intrinsic :: iso_c_binding
  use ftte_binding
  implicit none

  integer(c_int32_t) :: n, ncell32, ns, maxpos
  integer(c_int64_t) :: ncell, nchanged
  type(c_ptr) :: ctx
  integer(c_int32_t), allocatable :: lev(:), slev(:), spos(:,:)
  integer(c_int64_t), allocatable :: host(:)
  real(c_double), allocatable :: med(:,:), outv(:,:)
  real(c_double) :: box
  character(len=512) :: caseName, outName
  integer :: ios, iStar

  call get_command_argument(1, caseName)
  call get_command_argument(2, outName)
  open(11, file=trim(caseName), access='stream', form='unformatted', status='old', iostat=ios)
  if (ios /= 0) stop 'ftte_demo_expansion: cannot open case file'
  read(11) n, ncell32, ns, maxpos
  read(11) box
  ncell = ncell32
  allocate(lev(ncell), med(ncell,4), outv(ncell,5), slev(ns), spos(maxpos,ns), host(ns))
  read(11) lev
  read(11) med
  read(11) slev
  read(11) spos
  close(11)

  call ftteCheck(c_null_ptr, ftte_create(ctx, 1, c_null_ptr), 'ftte_create')
  call ftteCheck(ctx, ftte_set_grid(ctx, n, n, n, ncell, lev, box), 'ftte_set_grid')
  ! (no dust approximation: abun2 is not read; rho stands in for it)
  call ftteCheck(ctx, ftte_set_medium(ctx, med(:,2), med(:,3), med(:,4), med(:,1), med(:,1), 0), 'ftte_set_medium')
  do iStar = 1, ns
     call ftteCheck(ctx, ftte_locate_cell(ctx, slev(iStar), spos(1:3*slev(iStar)+3,iStar), host(iStar)), 'ftte_locate_cell')
  enddo
  call ftteCheck(ctx, ftte_expand_hii_regions(ctx, ns, host, c_null_ptr, outv(:,1), nchanged), 'ftte_expand_hii_regions')
  call ftteCheck(ctx, ftte_get_density(ctx, outv(:,2)), 'ftte_get_density')
  call ftteCheck(ctx, ftte_get_medium(ctx, outv(:,3), outv(:,4), outv(:,5)), 'ftte_get_medium')

  open(12, file=trim(outName), access='stream', form='unformatted', status='replace')
  write(12) outv
  close(12)
  write(*,'(a,i4,a,i9,a,i6,a,i9,a,i12)') ' grid ', n, '^3 base, ', ncell, ' cells, ', ns, ' stars, ', nchanged, &
       ' leaves changed, exact tests ', ftte_counter(ctx, 'expansion_exact_tests'//c_null_char)
  write(*,*) 'ftte_demo_expansion OK'
  call ftteCheck(ctx, ftte_destroy(ctx), 'ftte_destroy')

end program ftte_demo_expansion
