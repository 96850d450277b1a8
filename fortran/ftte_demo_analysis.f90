! ftte_demo_analysis.f90 -- a Fortran host for the analysis modes, through ftte_binding, without the reference's modules: the
! clumping line as mode clumpingFactor prints it (equiSources.f90:674), the reader's slice map of HI (readCellArray.f90:116-140) and
! the mass-weighted projection of abun2 of mode initialConfiguration (equiSources.f90:678-719), the maps as raw float32 in the
! order of mapArray(nxmap,nymap) -- what the reference hands to its HDF4 writer.
!
!   ftte_demo_analysis <case.bin> <out.bin>
!
! case.bin (stream): int32 n, ncell, izone, nxmap, nymap ; real64 box, zslice, centre(3), zoom ; int32 level(ncell) ;
!   real64 rho, abun2, HI (ncell each)
! out.bin: real32 slice(nxmap,nymap), projection(nxmap,nymap) ; real64 clumping, volume, mean_nh
program ftte_demo_analysis

  use, intrinsic :: iso_c_binding
  use ftte_binding
  implicit none

  integer(c_int32_t) :: n, ncell32, izone, nxmap, nymap
  integer(c_int64_t) :: ncell
  type(c_ptr) :: ctx
  integer(c_int32_t), allocatable :: lev(:)
  real(c_double), allocatable :: med(:,:)
  real(c_float), allocatable :: sliceMap(:,:), projectedMap(:,:)
  real(c_double) :: box, zslice, centre(3), zoom, clumping, volSum, meanDensity
  character(len=512) :: caseName, outName
  integer :: ios

  call get_command_argument(1, caseName)
  call get_command_argument(2, outName)
  open(11, file=trim(caseName), access='stream', form='unformatted', status='old', iostat=ios)
  if (ios /= 0) stop 'ftte_demo_analysis: cannot open case file'
  read(11) n, ncell32, izone, nxmap, nymap
  read(11) box, zslice, centre, zoom
  ncell = ncell32
  allocate(lev(ncell), med(ncell,3), sliceMap(nxmap,nymap), projectedMap(nxmap,nymap))
  read(11) lev
  read(11) med
  close(11)

  call ftteCheck(c_null_ptr, ftte_create(ctx, 1, c_null_ptr), 'ftte_create')
  call ftteCheck(ctx, ftte_set_grid(ctx, n, n, n, ncell, lev, box), 'ftte_set_grid')
  ! (the maps and the census read HI, rho and abun2; HI stands in for the helium species)
  call ftteCheck(ctx, ftte_set_medium(ctx, med(:,3), med(:,3), med(:,3), med(:,1), med(:,2), 0), 'ftte_set_medium')

  call ftteCheck(ctx, ftte_clumping(ctx, clumping, volSum, meanDensity), 'ftte_clumping')
  print*, 'clumping =', clumping, volSum
  call ftteCheck(ctx, ftte_slice_map(ctx, izone, nxmap, nymap, centre(1:2), zoom, zslice, c_null_ptr, sliceMap), 'ftte_slice_map')
  call ftteCheck(ctx, ftte_project_map(ctx, izone, nxmap, nymap, centre, zoom, 0, c_null_ptr, projectedMap), 'ftte_project_map')

  open(12, file=trim(outName), access='stream', form='unformatted', status='replace')
  write(12) sliceMap, projectedMap
  write(12) clumping, volSum, meanDensity
  close(12)
  write(*,*) 'ftte_demo_analysis OK'
  call ftteCheck(ctx, ftte_destroy(ctx), 'ftte_destroy')

end program ftte_demo_analysis
