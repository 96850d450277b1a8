! ftte_demo_evolve.f90 -- a Fortran host for time-dependent ionisation on the GPU: the reference's outer iteration
! (equiSources.f90:1230-1843) as ftte_demo_loop runs it, with solveRateEquations replaced by the advance over a time step and a
! time variable beside the iteration count: per step
!     setZeroRates -> star loop (ftte_point_sources) -> computeOpacities (ftte_compute_opacities) ->
!     diffuse sweep over 12*4**(L-1) directions (ftte_diffuse_sweep) -> ftte_advance_rate_equations over dt -> computeMass
! The rates and J of a step are those of the state at its start (explicit coupling); the chemistry over dt is implicit.
!
!   ftte_demo_evolve <case.bin> <out.bin> <dt in seconds> [substeps]
!
! case.bin: as ftte_demo_loop's (niter is the number of steps)
! out.bin: real64 HI, HeI, HeII (ncell each) after the last step ; real64 J(ncell,3) of the last sweep ;
!   real64 time(0:niter) ; real64 neutralFraction(0:niter)
program ftte_demo_evolve

  use, intrinsic :: iso_c_binding
  use ftte_binding
  implicit none

  integer(c_int32_t) :: n, ncell32, nsrc, niter, angularLevel, nratec
  integer(c_int64_t) :: ncell, ipix
  integer(c_int) :: highest, ndir, i, it, substeps
  type(c_ptr) :: ctx
  integer(c_int32_t), allocatable :: lev(:)
  integer(c_int64_t), allocatable :: src(:)
  real(c_double), allocatable :: gas(:,:), ndot(:), tables(:), k(:,:), J(:,:), phi(:), theta(:), w(:), species(:,:)
  real(c_double), allocatable :: time(:), neutralFraction(:)
  real(c_double) :: box, alpha(3), uvb(3), logtem(3), beta(3,3), ksi(3,3), gam(3,3), uniform(3), change, dt
  real(c_double) :: neutralHydrogenMass, totalHydrogenMass
  character(len=512) :: caseName, outName, word
  integer :: ios

  call get_command_argument(1, caseName)
  call get_command_argument(2, outName)
  call get_command_argument(3, word)
  read(word, *, iostat=ios) dt
  if (ios /= 0) stop 'ftte_demo_evolve: usage: ftte_demo_evolve <case.bin> <out.bin> <dt in seconds> [substeps]'
  substeps = 1
  if (command_argument_count() >= 4) then
     call get_command_argument(4, word)
     read(word, *, iostat=ios) substeps
     if (ios /= 0) stop 'ftte_demo_evolve: substeps is not a number'
  endif

  open(11, file=trim(caseName), access='stream', form='unformatted', status='old', iostat=ios)
  if (ios /= 0) stop 'ftte_demo_evolve: cannot open case file'
  read(11) n, ncell32, nsrc, niter, angularLevel, nratec
  read(11) box, alpha, uvb
  ncell = ncell32
  allocate(lev(ncell), gas(ncell,5), src(nsrc), ndot(nsrc), tables(6*11**4), k(nratec,6), J(ncell,3), species(ncell,3))
  allocate(time(0:niter), neutralFraction(0:niter))
  read(11) lev
  read(11) gas
  read(11) src
  read(11) ndot
  read(11) tables
  read(11) logtem
  read(11) k
  close(11)

  ! the direction loop header of the reference, equiSources.f90:1385-1391
  ndir = 12 * 4**(angularLevel-1)
  allocate(phi(ndir), theta(ndir), w(ndir))
  do i = 1, ndir
     ipix = i - 1
     if (ftte_pix2ang_nest(2**(angularLevel-1), ipix, phi(i), theta(i)) /= FTTE_OK) stop 'pix2ang_nest failed'
  enddo
  w = 1./float(ndir)
  uniform = 0.d0
  J = 0.d0

  call ftteCheck(c_null_ptr, ftte_create(ctx, 1, c_null_ptr), 'ftte_create')
  call ftteCheck(ctx, ftte_uvb_beta_table(400, real(0.02, c_double), alpha, beta, ksi, gam), 'ftte_uvb_beta_table')
  call ftteCheck(ctx, ftte_set_grid(ctx, n, n, n, ncell, lev, box), 'ftte_set_grid')
  call ftteCheck(ctx, ftte_set_rate_tables(ctx, tables), 'ftte_set_rate_tables')
  call ftteCheck(ctx, ftte_set_rate_coefficients(ctx, nratec, logtem(1), logtem(2), logtem(3), k(:,1), k(:,2), k(:,3), k(:,4), &
       k(:,5), k(:,6)), 'ftte_set_rate_coefficients')
  call ftteCheck(ctx, ftte_set_medium(ctx, gas(:,3), gas(:,4), gas(:,5), gas(:,1), gas(:,1), 0), 'ftte_set_medium')
  call ftteCheck(ctx, ftte_set_temperature(ctx, gas(:,2)), 'ftte_set_temperature')

  time(0) = 0.d0
  call ftteCheck(ctx, ftte_hydrogen_mass(ctx, neutralHydrogenMass, totalHydrogenMass), 'ftte_hydrogen_mass')
  neutralFraction(0) = neutralHydrogenMass / totalHydrogenMass
  do it = 1, niter
     call ftteCheck(ctx, ftte_set_zero_rates(ctx), 'ftte_set_zero_rates')
     call ftteCheck(ctx, ftte_point_sources(ctx, nsrc, src, ndot, highest), 'ftte_point_sources')
     call ftteCheck(ctx, ftte_compute_opacities(ctx, 3, beta), 'ftte_compute_opacities')
     call ftteCheck(ctx, ftte_diffuse_sweep(ctx, ndir, phi, theta, w, uvb, J), 'ftte_diffuse_sweep')
     call ftteCheck(ctx, ftte_advance_rate_equations(ctx, dt, substeps, 1, J, ksi, uniform, 0.d0, 1, change), &
          'ftte_advance_rate_equations')
     time(it) = it * dt
     call ftteCheck(ctx, ftte_hydrogen_mass(ctx, neutralHydrogenMass, totalHydrogenMass), 'ftte_hydrogen_mass')
     neutralFraction(it) = neutralHydrogenMass / totalHydrogenMass
     write(*,'(a,i4,a,es12.4,a,es14.6,a,es12.4)') ' step ', it, ': time ', time(it), ' s, neutral hydrogen fraction ', &
          neutralFraction(it), ', largest change of a species fraction ', change
  enddo
  call ftteCheck(ctx, ftte_get_medium(ctx, species(:,1), species(:,2), species(:,3)), 'ftte_get_medium')

  open(12, file=trim(outName), access='stream', form='unformatted', status='replace')
  write(12) species
  write(12) J
  write(12) time
  write(12) neutralFraction
  close(12)
  write(*,*) 'ftte_demo_evolve OK'
  call ftteCheck(ctx, ftte_destroy(ctx), 'ftte_destroy')

end program ftte_demo_evolve
