! ftte_binding.f90 -- ISO_C_BINDING view of include/ftte.h for the Fortran host.
!
! The reference is a Fortran program; its diffuse-transfer block (equiSources.f90:1372-1808) is
! replaced by calls into libftte.so through these interfaces.  Nothing here computes: it is the
! thin shim the north star asks for.  Status codes are those of ftte_status in ftte.h; the
! wrapper `ftteCheck` reproduces the reference's behaviour on inconsistency (`write; stop`).
module ftte_binding

  use, intrinsic :: iso_c_binding
  implicit none

  integer(c_int), parameter :: FTTE_OK = 0

  interface

     integer(c_int) function ftte_create(ctx, ndev, dev_ids) bind(C, name='ftte_create')
       import :: c_ptr, c_int
       type(c_ptr), intent(out) :: ctx
       integer(c_int), value :: ndev
       type(c_ptr), value :: dev_ids            ! const int*, may be c_null_ptr
     end function ftte_create

     integer(c_int) function ftte_destroy(ctx) bind(C, name='ftte_destroy')
       import :: c_ptr, c_int
       type(c_ptr), value :: ctx
     end function ftte_destroy

     type(c_ptr) function ftte_last_error(ctx) bind(C, name='ftte_last_error')
       import :: c_ptr
       type(c_ptr), value :: ctx
     end function ftte_last_error

     type(c_ptr) function ftte_multi_info(ctx) bind(C, name='ftte_multi_info')
       import :: c_ptr
       type(c_ptr), value :: ctx
     end function ftte_multi_info

     integer(c_int) function ftte_set_grid(ctx, nx, ny, nz, ncell, level, box_cm) bind(C, name='ftte_set_grid')
       import :: c_ptr, c_int, c_int64_t, c_int32_t, c_double
       type(c_ptr), value :: ctx
       integer(c_int), value :: nx, ny, nz
       integer(c_int64_t), value :: ncell
       integer(c_int32_t), intent(in) :: level(*)
       real(c_double), value :: box_cm
     end function ftte_set_grid

     integer(c_int) function ftte_set_opacity(ctx, nnu, kappa) bind(C, name='ftte_set_opacity')
       import :: c_ptr, c_int, c_double
       type(c_ptr), value :: ctx
       integer(c_int), value :: nnu
       real(c_double), intent(in) :: kappa(*)   ! (ncell, nnu) in Fortran order == [nnu][ncell] in C
     end function ftte_set_opacity

     integer(c_int) function ftte_set_species(ctx, nnu, HI, HeI, HeII, beta) bind(C, name='ftte_set_species')
       import :: c_ptr, c_int, c_double
       type(c_ptr), value :: ctx
       integer(c_int), value :: nnu
       real(c_double), intent(in) :: HI(*), HeI(*), HeII(*)
       real(c_double), intent(in) :: beta(*)    ! (nnu, 3) in Fortran order == [3][nnu] in C
     end function ftte_set_species

     integer(c_int) function ftte_set_emissivity(ctx, eta) bind(C, name='ftte_set_emissivity')
       import :: c_ptr, c_int
       type(c_ptr), value :: ctx
       type(c_ptr), value :: eta                ! const double* (ncell, nnu); c_null_ptr: the reference's zero emissivity
     end function ftte_set_emissivity

     integer(c_int) function ftte_set_source_function(ctx, S) bind(C, name='ftte_set_source_function')
       import :: c_ptr, c_int
       type(c_ptr), value :: ctx
       type(c_ptr), value :: S                  ! const double* (ncell, nnu), or c_null_ptr: emission off
     end function ftte_set_source_function

     integer(c_int) function ftte_diffuse_sweep(ctx, ndir, phi, theta, w, uvb, J) bind(C, name='ftte_diffuse_sweep')
       import :: c_ptr, c_int, c_double
       type(c_ptr), value :: ctx
       integer(c_int), value :: ndir
       real(c_double), intent(in) :: phi(*), theta(*), w(*), uvb(*)
       real(c_double), intent(out) :: J(*)      ! (ncell, nnu)
     end function ftte_diffuse_sweep

     ! The diagonal of the Lambda operator of the sweep with a source function (the build's own definition, not in the reference):
     ! diag(cell, nu) = J(cell) of a sweep with S = 1 in that cell alone and no inflow.  Stale after a new grid, new opacities or
     ! another direction list.
     integer(c_int) function ftte_lambda_diagonal(ctx, ndir, phi, theta, w, diag) bind(C, name='ftte_lambda_diagonal')
       import :: c_ptr, c_int, c_double
       type(c_ptr), value :: ctx
       integer(c_int), value :: ndir
       real(c_double), intent(in) :: phi(*), theta(*), w(*)
       real(c_double), intent(out) :: diag(*)   ! (ncell, nnu)
     end function ftte_lambda_diagonal

     integer(c_int) function ftte_lambda_diagonal_device(ctx, ndir, phi, theta, w, diag_dev, stream) &
          bind(C, name='ftte_lambda_diagonal_device')
       import :: c_ptr, c_int, c_double
       type(c_ptr), value :: ctx
       integer(c_int), value :: ndir
       real(c_double), intent(in) :: phi(*), theta(*), w(*)
       type(c_ptr), value :: diag_dev           ! double* in device memory (ncell, nnu)
       type(c_ptr), value :: stream             ! hipStream_t, or c_null_ptr: the context's own
     end function ftte_lambda_diagonal_device

     ! S <- S + ((1 - eps) J + eps B - S) / (1 - (1 - eps) diag) on device arrays (diag_dev = c_null_ptr: S <- (1 - eps) J + eps B);
     ! change = (max |S_new - S_old|, max |S_new|)
     integer(c_int) function ftte_source_update_device(ctx, nnu, epsilon, B_dev, b_per_cell, J_dev, diag_dev, S_dev, change, stream) &
          bind(C, name='ftte_source_update_device')
       import :: c_ptr, c_int, c_double
       type(c_ptr), value :: ctx
       integer(c_int), value :: nnu, b_per_cell
       real(c_double), value :: epsilon
       type(c_ptr), value :: B_dev, J_dev, diag_dev, S_dev   ! device memory; B (nnu), or (ncell, nnu) with b_per_cell = 1
       real(c_double), intent(out) :: change(2)
       type(c_ptr), value :: stream
     end function ftte_source_update_device

     ! ftte_set_opacity + ftte_diffuse_sweep in one call; on a uniform grid the groups cross PCIe and are swept in overlapping lanes
     integer(c_int) function ftte_diffuse_iteration(ctx, nnu, kappa, ndir, phi, theta, w, uvb, J) bind(C, name='ftte_diffuse_iteration')
       import :: c_ptr, c_int, c_double
       type(c_ptr), value :: ctx
       integer(c_int), value :: nnu, ndir
       real(c_double), intent(in) :: kappa(*)   ! (ncell, nnu)
       real(c_double), intent(in) :: phi(*), theta(*), w(*), uvb(*)
       real(c_double), intent(out) :: J(*)      ! (ncell, nnu)
     end function ftte_diffuse_iteration

     ! pins a host array the caller keeps (kappa, J): moved by DMA without a staging copy while it stays registered
     integer(c_int) function ftte_host_register(ctx, ptr, bytes) bind(C, name='ftte_host_register')
       import :: c_ptr, c_int, c_size_t
       type(c_ptr), value :: ctx, ptr
       integer(c_size_t), value :: bytes
     end function ftte_host_register

     integer(c_int) function ftte_host_unregister(ctx, ptr) bind(C, name='ftte_host_unregister')
       import :: c_ptr, c_int
       type(c_ptr), value :: ctx, ptr
     end function ftte_host_unregister

     ! "grid_builds", "plan_builds", "forest_builds" (null-terminated): how often the host-side builds ran
     integer(c_long_long) function ftte_counter(ctx, name) bind(C, name='ftte_counter')
       import :: c_ptr, c_long_long, c_char
       type(c_ptr), value :: ctx
       character(kind=c_char), intent(in) :: name(*)
     end function ftte_counter

     integer(c_int) function ftte_set_option(ctx, key, val) bind(C, name='ftte_set_option')
       import :: c_ptr, c_int, c_char
       type(c_ptr), value :: ctx
       character(kind=c_char), intent(in) :: key(*)
       integer(c_int), value :: val
     end function ftte_set_option

     integer(c_int) function ftte_pix2ang_nest(nside, ipix, phi, theta) bind(C, name='ftte_pix2ang_nest')
       import :: c_int, c_int64_t, c_double
       integer(c_int), value :: nside
       integer(c_int64_t), value :: ipix
       real(c_double), intent(out) :: phi, theta
     end function ftte_pix2ang_nest

     integer(c_int) function ftte_fold_direction(phi_large, theta_large, phi, theta, izone) bind(C, name='ftte_fold_direction')
       import :: c_int, c_double
       real(c_double), value :: phi_large, theta_large
       real(c_double), intent(out) :: phi, theta
       integer(c_int), intent(out) :: izone
     end function ftte_fold_direction

     integer(c_int) function ftte_rotate_indices(i, j, k, nx, ny, nz, izone, icell, jcell, kcell) &
          bind(C, name='ftte_rotate_indices')
       import :: c_int
       integer(c_int), value :: i, j, k, nx, ny, nz, izone
       integer(c_int), intent(out) :: icell, jcell, kcell
     end function ftte_rotate_indices

     ! ---- point sources (the runStellarTransfer block, equiSources.f90:1256-1370)

     integer(c_int) function ftte_stellar_beta_table(ctx, a_smc, nwave, wavelength_cm, nspectrum, nmetal, &
          specific_luminosity, iSpectrum, coefSpectrum, iMetal, coefMetal, total_integral) &
          bind(C, name='ftte_stellar_beta_table')
       import :: c_ptr, c_int, c_double
       type(c_ptr), value :: ctx
       real(c_double), intent(in) :: a_smc(7,5)               ! module dust
       integer(c_int), value :: nwave, nspectrum, nmetal
       real(c_double), intent(in) :: wavelength_cm(*)         ! wavelength(nWavelengths)
       real(c_double), intent(in) :: specific_luminosity(*)   ! specificLuminosity(nMetallicity,nSpectra,nWavelengths), as is
       integer(c_int), value :: iSpectrum, iMetal
       real(c_double), value :: coefSpectrum, coefMetal
       real(c_double), intent(out) :: total_integral
     end function ftte_stellar_beta_table

     ! population slots: npop table sets side by side for ftte_point_sources_populations; the four population arrays (npop)
     integer(c_int) function ftte_stellar_beta_tables(ctx, a_smc, nwave, wavelength_cm, nspectrum, nmetal, &
          specific_luminosity, npop, iSpectrum, coefSpectrum, iMetal, coefMetal, total_integral) &
          bind(C, name='ftte_stellar_beta_tables')
       import :: c_ptr, c_int, c_double
       type(c_ptr), value :: ctx
       real(c_double), intent(in) :: a_smc(7,5)
       integer(c_int), value :: nwave, nspectrum, nmetal, npop
       real(c_double), intent(in) :: wavelength_cm(*)
       real(c_double), intent(in) :: specific_luminosity(*)
       integer(c_int), intent(in) :: iSpectrum(*), iMetal(*)
       real(c_double), intent(in) :: coefSpectrum(*), coefMetal(*)
       real(c_double), intent(out) :: total_integral(*)
     end function ftte_stellar_beta_tables

     integer(c_int) function ftte_set_population_tables(ctx, npop, tables) bind(C, name='ftte_set_population_tables')
       import :: c_ptr, c_int, c_double
       type(c_ptr), value :: ctx
       integer(c_int), value :: npop
       real(c_double), intent(in) :: tables(*)   ! npop sets as for ftte_set_rate_tables, one after the other
     end function ftte_set_population_tables

     integer(c_int) function ftte_get_population_tables(ctx, slot, tables) bind(C, name='ftte_get_population_tables')
       import :: c_ptr, c_int, c_double
       type(c_ptr), value :: ctx
       integer(c_int), value :: slot             ! 0-based
       real(c_double), intent(out) :: tables(*)
     end function ftte_get_population_tables

     integer(c_int) function ftte_set_rate_tables(ctx, tables) bind(C, name='ftte_set_rate_tables')
       import :: c_ptr, c_int, c_double
       type(c_ptr), value :: ctx
       real(c_double), intent(in) :: tables(*)   ! reactionRate1..3, energyRate1..3, each (0:10,0:10,0:10,0:10)
     end function ftte_set_rate_tables

     integer(c_int) function ftte_get_rate_tables(ctx, tables) bind(C, name='ftte_get_rate_tables')
       import :: c_ptr, c_int, c_double
       type(c_ptr), value :: ctx
       real(c_double), intent(out) :: tables(*)
     end function ftte_get_rate_tables

     integer(c_int) function ftte_get_rates_hydrogen_helium(ctx, dust_approximation, nsample, tau, rates) &
          bind(C, name='ftte_get_rates_hydrogen_helium')
       import :: c_ptr, c_int, c_double
       type(c_ptr), value :: ctx
       integer(c_int), value :: dust_approximation, nsample
       real(c_double), intent(in) :: tau(*)      ! (4, nsample)
       real(c_double), intent(out) :: rates(*)   ! (2, 3, nsample): numberRate, heatingRate per reaction
     end function ftte_get_rates_hydrogen_helium

     integer(c_int) function ftte_set_medium(ctx, HI, HeI, HeII, rho, abun2, dust_approximation) &
          bind(C, name='ftte_set_medium')
       import :: c_ptr, c_int, c_double
       type(c_ptr), value :: ctx
       real(c_double), intent(in) :: HI(*), HeI(*), HeII(*), rho(*), abun2(*)
       integer(c_int), value :: dust_approximation
     end function ftte_set_medium

     integer(c_int) function ftte_set_zero_rates(ctx) bind(C, name='ftte_set_zero_rates')
       import :: c_ptr, c_int
       type(c_ptr), value :: ctx
     end function ftte_set_zero_rates

     integer(c_int) function ftte_locate_cell(ctx, level, position, cell) bind(C, name='ftte_locate_cell')
       import :: c_ptr, c_int, c_int32_t, c_int64_t
       type(c_ptr), value :: ctx
       integer(c_int), value :: level
       integer(c_int32_t), intent(in) :: position(*)   ! starType%position(1:3*level+3)
       integer(c_int64_t), intent(out) :: cell         ! 0-based cell-array index
     end function ftte_locate_cell

     ! ---- the star catalogue: equiSources.f90:746-769 and :1169-1212 on the device, :1282-1293 on the host.  Stars are merged by
     ! host leaf (include/ftte.h).  xyz(3,nstars) in the units of lo, hi; weight(nstars) >= 0 or c_null_ptr (1 each); star_cell(nstars)
     ! 0-based host leaf, -1 outside the box, or c_null_ptr
     integer(c_int) function ftte_star_catalogue(ctx, nstars, xyz, lo, hi, weight, star_cell, nsrc, outside) &
          bind(C, name='ftte_star_catalogue')
       import :: c_ptr, c_int, c_int64_t, c_double
       type(c_ptr), value :: ctx
       integer(c_int64_t), value :: nstars
       real(c_double), intent(in) :: xyz(*), lo(3), hi(3)
       type(c_ptr), value :: weight, star_cell
       integer(c_int64_t), intent(out) :: nsrc, outside
     end function ftte_star_catalogue

     ! the sources of the last ftte_star_catalogue, ascending src_cell; every array may be c_null_ptr: src_cell (int64),
     ! src_weight (int32), src_ndot (real64), src_first_star (int64, 0-based), src_abun2 (real64; needs a medium with abun2)
     integer(c_int) function ftte_star_sources(ctx, nsrc, src_cell, src_weight, src_ndot, src_first_star, src_abun2) &
          bind(C, name='ftte_star_sources')
       import :: c_ptr, c_int, c_int64_t
       type(c_ptr), value :: ctx
       integer(c_int64_t), value :: nsrc
       type(c_ptr), value :: src_cell, src_weight, src_ndot, src_first_star, src_abun2
     end function ftte_star_sources

     ! host only: (iMetal, coefMetal) per source and one population slot (0-based) per distinct pair; pop_first(npop) 0-based
     integer(c_int) function ftte_star_populations(nmetal, metallicity, nsrc, abun2, iMetal, coefMetal, src_slot, npop, pop_first) &
          bind(C, name='ftte_star_populations')
       import :: c_int, c_int32_t, c_int64_t, c_double
       integer(c_int), value :: nmetal
       real(c_double), intent(in) :: metallicity(*), abun2(*)
       integer(c_int64_t), value :: nsrc
       integer(c_int32_t), intent(out) :: iMetal(*), src_slot(*)
       real(c_double), intent(out) :: coefMetal(*)
       integer(c_int64_t), intent(out) :: npop, pop_first(*)
     end function ftte_star_populations

     ! host only: the inverse of ftte_locate_cell; position needs 3*(level+1) entries, 183 always suffice
     integer(c_int) function ftte_cell_position(ctx, cell, level, position) bind(C, name='ftte_cell_position')
       import :: c_ptr, c_int, c_int32_t, c_int64_t
       type(c_ptr), value :: ctx
       integer(c_int64_t), value :: cell
       integer(c_int), intent(out) :: level
       integer(c_int32_t), intent(out) :: position(*)
     end function ftte_cell_position

     integer(c_int) function ftte_point_sources(ctx, nsrc, src_cell, src_ndot, highest_pixel_level) &
          bind(C, name='ftte_point_sources')
       import :: c_ptr, c_int, c_int64_t, c_double
       type(c_ptr), value :: ctx
       integer(c_int), value :: nsrc
       integer(c_int64_t), intent(in) :: src_cell(*)
       real(c_double), intent(in) :: src_ndot(*)
       integer(c_int), intent(out) :: highest_pixel_level
     end function ftte_point_sources

     ! star s reads population slot src_slot(s) (0-based); highest_pixel_level(nsrc) is per star
     integer(c_int) function ftte_point_sources_populations(ctx, nsrc, src_cell, src_ndot, src_slot, highest_pixel_level) &
          bind(C, name='ftte_point_sources_populations')
       import :: c_ptr, c_int, c_int32_t, c_int64_t, c_double
       type(c_ptr), value :: ctx
       integer(c_int), value :: nsrc
       integer(c_int64_t), intent(in) :: src_cell(*)
       real(c_double), intent(in) :: src_ndot(*)
       integer(c_int32_t), intent(in) :: src_slot(*)
       integer(c_int), intent(out) :: highest_pixel_level(*)
     end function ftte_point_sources_populations

     ! escape bookkeeping of the last ftte_point_sources / ftte_point_sources_populations call (equiSources.f90:3198-3233, 1342-1348); arrays as Fortran
     ! (7,nsrc), (7,nsrc), (nsrc), (300,nsrc), (7,nsrc); pass c_null_ptr-associated dummies by using the _opt variant if unwanted
     integer(c_int) function ftte_point_escape(ctx, nsrc, remaining, boundary, dust, spectrum, fraction) bind(C, name='ftte_point_escape')
       import :: c_ptr, c_int, c_double
       type(c_ptr), value :: ctx
       integer(c_int), value :: nsrc
       real(c_double), intent(out) :: remaining(*), boundary(*), dust(*), spectrum(*), fraction(*)
     end function ftte_point_escape

     integer(c_int) function ftte_set_output_sigma(ctx, sigma) bind(C, name='ftte_set_output_sigma')
       import :: c_ptr, c_int, c_double
       type(c_ptr), value :: ctx
       real(c_double), intent(in) :: sigma(*)
     end function ftte_set_output_sigma

     integer(c_int) function ftte_get_point_rates(ctx, rates) bind(C, name='ftte_get_point_rates')
       import :: c_ptr, c_int, c_double
       type(c_ptr), value :: ctx
       real(c_double), intent(out) :: rates(*)   ! (ncell, 6): krate24, krate25, krate26, crate24, crate25, crate26
     end function ftte_get_point_rates

     integer(c_int) function ftte_rmax(rmax30) bind(C, name='ftte_rmax')
       import :: c_int, c_double
       real(c_double), intent(out) :: rmax30(30)
     end function ftte_rmax

     real(c_double) function ftte_dust_cross_section(lambda_micron, a_smc) bind(C, name='ftte_dust_cross_section')
       import :: c_double
       real(c_double), value :: lambda_micron
       real(c_double), intent(in) :: a_smc(7,5)
     end function ftte_dust_cross_section

     ! ---- ionisation equilibrium (solveRateEquations, equiSources.f90:3459-3677)

     integer(c_int) function ftte_set_rate_coefficients(ctx, nratec, logtem0, logtem9, dlogtem, k1a, k2a, k3a, k4a, k5a, k6a) &
          bind(C, name='ftte_set_rate_coefficients')
       import :: c_ptr, c_int, c_double
       type(c_ptr), value :: ctx
       integer(c_int), value :: nratec
       real(c_double), value :: logtem0, logtem9, dlogtem
       real(c_double), intent(in) :: k1a(*), k2a(*), k3a(*), k4a(*), k5a(*), k6a(*)
     end function ftte_set_rate_coefficients

     integer(c_int) function ftte_set_temperature(ctx, tgas) bind(C, name='ftte_set_temperature')
       import :: c_ptr, c_int, c_double
       type(c_ptr), value :: ctx
       real(c_double), intent(in) :: tgas(*)
     end function ftte_set_temperature

     integer(c_int) function ftte_solve_rate_equations(ctx, run_uvb_transfer, J, ksi, uniform, self_shielding_threshold, &
          use_point_rates, max_change) bind(C, name='ftte_solve_rate_equations')
       import :: c_ptr, c_int, c_double
       type(c_ptr), value :: ctx
       integer(c_int), value :: run_uvb_transfer, use_point_rates
       real(c_double), intent(in) :: J(*)          ! (ncell, 3): Jmean1..3
       real(c_double), intent(in) :: ksi(3,3)      ! (ksi24, ksi25, ksi26) x (group1, group2, group3)
       real(c_double), intent(in) :: uniform(3)
       real(c_double), value :: self_shielding_threshold
       real(c_double), intent(out) :: max_change
     end function ftte_solve_rate_equations

     ! time-dependent ionisation: the species advanced over dt_s seconds in `substeps` implicit steps at the rates of the state on
     ! entry, instead of replaced by their equilibrium; the other arguments as ftte_solve_rate_equations
     integer(c_int) function ftte_advance_rate_equations(ctx, dt_s, substeps, run_uvb_transfer, J, ksi, uniform, &
          self_shielding_threshold, use_point_rates, max_change) bind(C, name='ftte_advance_rate_equations')
       import :: c_ptr, c_int, c_double
       type(c_ptr), value :: ctx
       real(c_double), value :: dt_s
       integer(c_int), value :: substeps, run_uvb_transfer, use_point_rates
       real(c_double), intent(in) :: J(*)          ! (ncell, 3): Jmean1..3
       real(c_double), intent(in) :: ksi(3,3)      ! (ksi24, ksi25, ksi26) x (group1, group2, group3)
       real(c_double), intent(in) :: uniform(3)
       real(c_double), value :: self_shielding_threshold
       real(c_double), intent(out) :: max_change
     end function ftte_advance_rate_equations

     ! same with J in device memory (e.g. what ftte_diffuse_sweep_device wrote)
     integer(c_int) function ftte_advance_rate_equations_device(ctx, dt_s, substeps, run_uvb_transfer, J_dev, ksi, uniform, &
          self_shielding_threshold, use_point_rates, max_change) bind(C, name='ftte_advance_rate_equations_device')
       import :: c_ptr, c_int, c_double
       type(c_ptr), value :: ctx
       real(c_double), value :: dt_s
       integer(c_int), value :: substeps, run_uvb_transfer, use_point_rates
       type(c_ptr), value :: J_dev
       real(c_double), intent(in) :: ksi(3,3)
       real(c_double), intent(in) :: uniform(3)
       real(c_double), value :: self_shielding_threshold
       real(c_double), intent(out) :: max_change
     end function ftte_advance_rate_equations_device

     integer(c_int) function ftte_get_medium(ctx, HI, HeI, HeII) bind(C, name='ftte_get_medium')
       import :: c_ptr, c_int, c_double
       type(c_ptr), value :: ctx
       real(c_double), intent(out) :: HI(*), HeI(*), HeII(*)
     end function ftte_get_medium

     ! equiSources.f90:1008-1022: initialIonizationEquilibrium `passes` times per leaf (the reference: 2) on the device-resident
     ! medium; neutral_fraction = neutralHydrogenMass / totalHydrogenMass of the result (what :1022 prints)
     integer(c_int) function ftte_initial_ionization_equilibrium(ctx, uniform, self_shielding_threshold, passes, neutral_fraction) &
          bind(C, name='ftte_initial_ionization_equilibrium')
       import :: c_ptr, c_int, c_double
       type(c_ptr), value :: ctx
       real(c_double), intent(in) :: uniform(3)
       real(c_double), value :: self_shielding_threshold
       integer(c_int), value :: passes
       real(c_double), intent(out) :: neutral_fraction
     end function ftte_initial_ionization_equilibrium

     ! computeMass (equiSources.f90:4369-4393) over the device-resident medium [msun]
     integer(c_int) function ftte_hydrogen_mass(ctx, neutral_msun, total_msun) bind(C, name='ftte_hydrogen_mass')
       import :: c_ptr, c_int, c_double
       type(c_ptr), value :: ctx
       real(c_double), intent(out) :: neutral_msun, total_msun
     end function ftte_hydrogen_mass

     ! computeExpansionParameters(nh), equiSources.f90:4395-4429 (host, no context)
     integer(c_int) function ftte_expansion_parameters(nh, final_radius_cm, density_coefficient) &
          bind(C, name='ftte_expansion_parameters')
       import :: c_int, c_double
       real(c_double), value :: nh
       real(c_double), intent(out) :: final_radius_cm, density_coefficient
     end function ftte_expansion_parameters

     ! equiSources.f90:1035-1069 (expansion of HII regions) on the device-resident medium: src_cell(nsrc) the host leaves of the
     ! stars with weight > 0 (ftte_locate_cell), params = c_null_ptr (computed from the host leaves' densities) or c_loc of
     ! params(3,nsrc) = finalRadius, densityCoefficient, sourceTotalHydrogenDensity; rho_coef(ncell) = rhoCoef
     integer(c_int) function ftte_expand_hii_regions(ctx, nsrc, src_cell, params, rho_coef, nchanged) &
          bind(C, name='ftte_expand_hii_regions')
       import :: c_ptr, c_int, c_int64_t, c_double
       type(c_ptr), value :: ctx
       integer(c_int), value :: nsrc
       integer(c_int64_t), intent(in) :: src_cell(*)
       type(c_ptr), value :: params
       real(c_double), intent(out) :: rho_coef(*)
       integer(c_int64_t), intent(out) :: nchanged
     end function ftte_expand_hii_regions

     ! rho of the device-resident medium
     integer(c_int) function ftte_get_density(ctx, rho) bind(C, name='ftte_get_density')
       import :: c_ptr, c_int, c_double
       type(c_ptr), value :: ctx
       real(c_double), intent(out) :: rho(*)
     end function ftte_get_density

     ! ---- analysis of the device-resident medium: the reader's slice map (readCellArray.f90:116-140), the projection of mode
     ! initialConfiguration (equiSources.f90:678-719), mode clumpingFactor (:661-676) and the PDFs of mode plotPDFs (:785-836)
     ! i0 and xnew of equiSources.f90:703-709 for the columns (or rows) of a projected map (host, no context)
     integer(c_int) function ftte_map_axis(n, nmap, centre, zoom, base, frac) bind(C, name='ftte_map_axis')
       import :: c_int, c_int32_t, c_double
       integer(c_int), value :: n, nmap
       real(c_double), value :: centre, zoom
       integer(c_int32_t), intent(out) :: base(*)
       real(c_double), intent(out) :: frac(*)
     end function ftte_map_axis

     ! the same for the reader's loops, readCellArray.f90:126-132 (host, no context)
     integer(c_int) function ftte_slice_axis(n, nmap, centre, zoom, base, frac) bind(C, name='ftte_slice_axis')
       import :: c_int, c_int32_t, c_double
       integer(c_int), value :: n, nmap
       real(c_double), value :: centre, zoom
       integer(c_int32_t), intent(out) :: base(*)
       real(c_double), intent(out) :: frac(*)
     end function ftte_slice_axis

     ! kstart and kend of equiSources.f90:687-700 (host, no context)
     integer(c_int) function ftte_map_depth(n, centre, zoom, kstart, kend) bind(C, name='ftte_map_depth')
       import :: c_int, c_int32_t, c_double
       integer(c_int), value :: n
       real(c_double), value :: centre, zoom
       integer(c_int32_t), intent(out) :: kstart, kend
     end function ftte_map_depth

     ! value: c_null_ptr (HI of the medium for a slice, abun2 for a projection) or c_loc of value(ncell); centre(2) / centre(3)
     integer(c_int) function ftte_slice_map(ctx, izone, nxmap, nymap, centre, zoom, zslice, value, map) &
          bind(C, name='ftte_slice_map')
       import :: c_ptr, c_int, c_double, c_float
       type(c_ptr), value :: ctx
       integer(c_int), value :: izone, nxmap, nymap
       real(c_double), intent(in) :: centre(*)
       real(c_double), value :: zoom
       real(c_double), value :: zslice
       type(c_ptr), value :: value           ! host array
       real(c_float), intent(out) :: map(*)  ! mapArray(nxmap,nymap)
     end function ftte_slice_map

     integer(c_int) function ftte_slice_map_device(ctx, izone, nxmap, nymap, centre, zoom, zslice, value, map) &
          bind(C, name='ftte_slice_map_device')
       import :: c_ptr, c_int, c_double, c_float
       type(c_ptr), value :: ctx
       integer(c_int), value :: izone, nxmap, nymap
       real(c_double), intent(in) :: centre(*)
       real(c_double), value :: zoom
       real(c_double), value :: zslice
       type(c_ptr), value :: value           ! device array
       real(c_float), intent(out) :: map(*)  ! mapArray(nxmap,nymap)
     end function ftte_slice_map_device

     ! mode 0: the reference's mass-weighted mean; 1: the path integral sum value * leaf size [cm] (not in the reference)
     integer(c_int) function ftte_project_map(ctx, izone, nxmap, nymap, centre, zoom, mode, value, map) &
          bind(C, name='ftte_project_map')
       import :: c_ptr, c_int, c_double, c_float
       type(c_ptr), value :: ctx
       integer(c_int), value :: izone, nxmap, nymap
       real(c_double), intent(in) :: centre(*)
       real(c_double), value :: zoom
       integer(c_int), value :: mode
       type(c_ptr), value :: value           ! host array
       real(c_float), intent(out) :: map(*)  ! mapArray(nxmap,nymap)
     end function ftte_project_map

     integer(c_int) function ftte_project_map_device(ctx, izone, nxmap, nymap, centre, zoom, mode, value, map) &
          bind(C, name='ftte_project_map_device')
       import :: c_ptr, c_int, c_double, c_float
       type(c_ptr), value :: ctx
       integer(c_int), value :: izone, nxmap, nymap
       real(c_double), intent(in) :: centre(*)
       real(c_double), value :: zoom
       integer(c_int), value :: mode
       type(c_ptr), value :: value           ! device array
       real(c_float), intent(out) :: map(*)  ! mapArray(nxmap,nymap)
     end function ftte_project_map_device

     ! equiSources.f90:661-676: clumping = volSumDensity2 / volSumDensity**2 after the division by volume = volSum
     integer(c_int) function ftte_clumping(ctx, clumping, volume, mean_nh) bind(C, name='ftte_clumping')
       import :: c_ptr, c_int, c_double
       type(c_ptr), value :: ctx
       real(c_double), intent(out) :: clumping, volume, mean_nh
     end function ftte_clumping

     ! pdfGas(npdf) and pdfGasOutside, equiSources.f90:814-822
     integer(c_int) function ftte_gas_pdf(ctx, pdf, outside) bind(C, name='ftte_gas_pdf')
       import :: c_ptr, c_int, c_double
       type(c_ptr), value :: ctx
       real(c_double), intent(out) :: pdf(50), outside
     end function ftte_gas_pdf

     ! pdfStar(npdf), pdfStarOutside and meanHostDensity/float(nStarsSpecificAge), :787-813; src_cell(nsrc) from ftte_locate_cell
     integer(c_int) function ftte_star_pdf(ctx, nsrc, src_cell, pdf, outside, mean_host_HI) bind(C, name='ftte_star_pdf')
       import :: c_ptr, c_int, c_int32_t, c_int64_t, c_double
       type(c_ptr), value :: ctx
       integer(c_int), value :: nsrc
       integer(c_int64_t), intent(in) :: src_cell(*)
       integer(c_int32_t), intent(out) :: pdf(50), outside
       real(c_double), intent(out) :: mean_host_HI
     end function ftte_star_pdf

     ! ---- absorption spectra along the projected map's pixel columns (not in the reference; include/ftte.h, csrc/ftte_spectra_math.h)
     ! velx, vely, velz: (ncell) each [cm/s] along storage i, j, k (c_loc of host arrays); three c_null_ptr drop the field
     integer(c_int) function ftte_set_velocity(ctx, velx, vely, velz) bind(C, name='ftte_set_velocity')
       import :: c_ptr, c_int
       type(c_ptr), value :: ctx
       type(c_ptr), value :: velx, vely, velz ! host arrays
     end function ftte_set_velocity

     integer(c_int) function ftte_set_velocity_device(ctx, velx, vely, velz) bind(C, name='ftte_set_velocity_device')
       import :: c_ptr, c_int
       type(c_ptr), value :: ctx
       type(c_ptr), value :: velx, vely, velz ! device arrays
     end function ftte_set_velocity_device

     ! line = (/ sigma_line, damping, mass, b_turb /); value: c_null_ptr = HI of the medium; tau(nvel,nxmap,nymap) and
     ! summary(3,nxmap,nymap) = N, W, dv90 as c_loc of host arrays, either one (not both) c_null_ptr
     integer(c_int) function ftte_sightline_spectra(ctx, izone, nxmap, nymap, centre, zoom, nvel, v0, dv, hubble, period, line, &
          value, tau, summary) bind(C, name='ftte_sightline_spectra')
       import :: c_ptr, c_int, c_double
       type(c_ptr), value :: ctx
       integer(c_int), value :: izone, nxmap, nymap
       real(c_double), intent(in) :: centre(3)
       real(c_double), value :: zoom
       integer(c_int), value :: nvel
       real(c_double), value :: v0, dv, hubble, period
       real(c_double), intent(in) :: line(4)
       type(c_ptr), value :: value, tau, summary ! host arrays
     end function ftte_sightline_spectra

     integer(c_int) function ftte_sightline_spectra_device(ctx, izone, nxmap, nymap, centre, zoom, nvel, v0, dv, hubble, period, &
          line, value, tau, summary) bind(C, name='ftte_sightline_spectra_device')
       import :: c_ptr, c_int, c_double
       type(c_ptr), value :: ctx
       integer(c_int), value :: izone, nxmap, nymap
       real(c_double), intent(in) :: centre(3)
       real(c_double), value :: zoom
       integer(c_int), value :: nvel
       real(c_double), value :: v0, dv, hubble, period
       real(c_double), intent(in) :: line(4)
       type(c_ptr), value :: value, tau, summary ! device arrays
     end function ftte_sightline_spectra_device

     ! the same along rays of any origin and direction: origin(3,nray), dir(3,nray) unit vectors in the storage frame, base cells;
     ! tmax(nray) as c_loc or c_null_ptr (to the box's far side); tau(nvel,nray), summary(3,nray); the rays are host arrays in both
     integer(c_int) function ftte_ray_spectra(ctx, nray, origin, dir, tmax, nvel, v0, dv, hubble, period, line, &
          value, tau, summary) bind(C, name='ftte_ray_spectra')
       import :: c_ptr, c_int, c_int64_t, c_double
       type(c_ptr), value :: ctx
       integer(c_int64_t), value :: nray
       real(c_double), intent(in) :: origin(3, *), dir(3, *)
       type(c_ptr), value :: tmax
       integer(c_int), value :: nvel
       real(c_double), value :: v0, dv, hubble, period
       real(c_double), intent(in) :: line(4)
       type(c_ptr), value :: value, tau, summary ! host arrays
     end function ftte_ray_spectra

     integer(c_int) function ftte_ray_spectra_device(ctx, nray, origin, dir, tmax, nvel, v0, dv, hubble, period, line, &
          value, tau, summary) bind(C, name='ftte_ray_spectra_device')
       import :: c_ptr, c_int, c_int64_t, c_double
       type(c_ptr), value :: ctx
       integer(c_int64_t), value :: nray
       real(c_double), intent(in) :: origin(3, *), dir(3, *)
       type(c_ptr), value :: tmax
       integer(c_int), value :: nvel
       real(c_double), value :: v0, dv, hubble, period
       real(c_double), intent(in) :: line(4)
       type(c_ptr), value :: value, tau, summary ! device arrays
     end function ftte_ray_spectra_device

     ! the rays' segment lists: offset(nray+1); leaf, t_in, t_out (capacity) as c_loc, or capacity 0 and c_null_ptr: the offsets alone
     integer(c_int) function ftte_ray_segments(ctx, nray, origin, dir, tmax, offset, capacity, leaf, t_in, t_out) &
          bind(C, name='ftte_ray_segments')
       import :: c_ptr, c_int, c_int64_t, c_double
       type(c_ptr), value :: ctx
       integer(c_int64_t), value :: nray
       real(c_double), intent(in) :: origin(3, *), dir(3, *)
       type(c_ptr), value :: tmax
       integer(c_int64_t), intent(out) :: offset(*)
       integer(c_int64_t), value :: capacity
       type(c_ptr), value :: leaf, t_in, t_out
     end function ftte_ray_segments

     ! the periodic namesakes: the box tiles space and a ray goes on through the opposite face from its origin (anywhere) to
     ! tmax(nray), which is required (c_loc) and > 0; t and s are measured from the caller's origin across images
     integer(c_int) function ftte_ray_spectra_periodic(ctx, nray, origin, dir, tmax, nvel, v0, dv, hubble, period, line, &
          value, tau, summary) bind(C, name='ftte_ray_spectra_periodic')
       import :: c_ptr, c_int, c_int64_t, c_double
       type(c_ptr), value :: ctx
       integer(c_int64_t), value :: nray
       real(c_double), intent(in) :: origin(3, *), dir(3, *)
       type(c_ptr), value :: tmax
       integer(c_int), value :: nvel
       real(c_double), value :: v0, dv, hubble, period
       real(c_double), intent(in) :: line(4)
       type(c_ptr), value :: value, tau, summary ! host arrays
     end function ftte_ray_spectra_periodic

     integer(c_int) function ftte_ray_spectra_periodic_device(ctx, nray, origin, dir, tmax, nvel, v0, dv, hubble, period, line, &
          value, tau, summary) bind(C, name='ftte_ray_spectra_periodic_device')
       import :: c_ptr, c_int, c_int64_t, c_double
       type(c_ptr), value :: ctx
       integer(c_int64_t), value :: nray
       real(c_double), intent(in) :: origin(3, *), dir(3, *)
       type(c_ptr), value :: tmax
       integer(c_int), value :: nvel
       real(c_double), value :: v0, dv, hubble, period
       real(c_double), intent(in) :: line(4)
       type(c_ptr), value :: value, tau, summary ! device arrays
     end function ftte_ray_spectra_periodic_device

     integer(c_int) function ftte_ray_segments_periodic(ctx, nray, origin, dir, tmax, offset, capacity, leaf, t_in, t_out) &
          bind(C, name='ftte_ray_segments_periodic')
       import :: c_ptr, c_int, c_int64_t, c_double
       type(c_ptr), value :: ctx
       integer(c_int64_t), value :: nray
       real(c_double), intent(in) :: origin(3, *), dir(3, *)
       type(c_ptr), value :: tmax
       integer(c_int64_t), intent(out) :: offset(*)
       integer(c_int64_t), value :: capacity
       type(c_ptr), value :: leaf, t_in, t_out
     end function ftte_ray_segments_periodic

     integer(c_int) function ftte_compute_opacities(ctx, nnu, beta) bind(C, name='ftte_compute_opacities')
       import :: c_ptr, c_int, c_double
       type(c_ptr), value :: ctx
       integer(c_int), value :: nnu
       real(c_double), intent(in) :: beta(*)       ! (nnu, 3)
     end function ftte_compute_opacities

     integer(c_int) function ftte_set_point_rates(ctx, rates) bind(C, name='ftte_set_point_rates')
       import :: c_ptr, c_int, c_double
       type(c_ptr), value :: ctx
       real(c_double), intent(in) :: rates(*)      ! (ncell, 6)
     end function ftte_set_point_rates

     integer(c_int) function ftte_uvb_beta_table(nfreq, freqdel, alpha, beta, ksi, gamma) bind(C, name='ftte_uvb_beta_table')
       import :: c_int, c_double
       integer(c_int), value :: nfreq
       real(c_double), value :: freqdel
       real(c_double), intent(in) :: alpha(3)
       real(c_double), intent(out) :: beta(3,3)    ! (group, species HI/HeI/HeII): the (nnu, 3) matrix of ftte_set_species
       real(c_double), intent(out) :: ksi(3,3)     ! (ksi24/25/26, group)
       real(c_double), intent(out) :: gamma(3,3)   ! (gammaHI/HeI/HeII, group)
     end function ftte_uvb_beta_table

     integer(c_int) function ftte_assign_uvb_radiation(ctx, nnu, uvb, self_shielding_threshold, J) &
          bind(C, name='ftte_assign_uvb_radiation')
       import :: c_ptr, c_int, c_double
       type(c_ptr), value :: ctx
       integer(c_int), value :: nnu
       real(c_double), intent(in) :: uvb(*)
       real(c_double), value :: self_shielding_threshold
       real(c_double), intent(out) :: J(*)         ! (ncell, nnu)
     end function ftte_assign_uvb_radiation

     integer(c_int) function ftte_uniform_table(nfreq, freqdel, alpha_quasar, alpha_stellar, ksi, gamma) &
          bind(C, name='ftte_uniform_table')
       import :: c_int, c_double
       integer(c_int), value :: nfreq
       real(c_double), value :: freqdel, alpha_quasar, alpha_stellar
       real(c_double), intent(out) :: ksi(3,2), gamma(3,2)   ! (24/25/26 or HI/HeI/HeII, quasar/stellar)
     end function ftte_uniform_table

     integer(c_int) function ftte_rate_coefficient_tables(nratec, temstart, temend, recombination_type, k, logtem0, logtem9, dlogtem) &
          bind(C, name='ftte_rate_coefficient_tables')
       import :: c_int, c_double
       integer(c_int), value :: nratec, recombination_type
       real(c_double), value :: temstart, temend
       real(c_double), intent(out) :: k(*)         ! (nratec, 6): k1a..k6a
       real(c_double), intent(out) :: logtem0, logtem9, dlogtem
     end function ftte_rate_coefficient_tables

     ! the thirteen cooling coefficients of calc_rates and compa; case B reads the caller's copies of the two data files (c_null_ptr
     ! for case A): mellema(2,81) = columns 1, 3 of HII-ktbetas.tab, gnedin(3,201) = columns 1, 3, 5 of cratesHe.res
     integer(c_int) function ftte_cooling_coefficient_tables(nratec, temstart, temend, recombination_type, mellema, gnedin, c, compa) &
          bind(C, name='ftte_cooling_coefficient_tables')
       import :: c_ptr, c_int, c_double
       integer(c_int), value :: nratec, recombination_type
       real(c_double), value :: temstart, temend
       type(c_ptr), value :: mellema, gnedin
       real(c_double), intent(out) :: c(*)         ! (nratec, 13): ceHIa .. lineHIa in the order of equiSources.f90:3975-3987
       real(c_double), intent(out) :: compa
     end function ftte_cooling_coefficient_tables

     ! ---- thermal balance: thermalEquilibrium (equiSources.f90:3870-4042) and the temperature advanced over a time step
     integer(c_int) function ftte_get_temperature(ctx, tgas) bind(C, name='ftte_get_temperature')
       import :: c_ptr, c_int, c_double
       type(c_ptr), value :: ctx
       real(c_double), intent(out) :: tgas(*)
     end function ftte_get_temperature

     integer(c_int) function ftte_set_cooling_coefficients(ctx, nratec, c, compa, redshift) bind(C, name='ftte_set_cooling_coefficients')
       import :: c_ptr, c_int, c_double
       type(c_ptr), value :: ctx
       integer(c_int), value :: nratec
       real(c_double), intent(in) :: c(*)          ! (nratec, 13)
       real(c_double), value :: compa, redshift
     end function ftte_set_cooling_coefficients

     ! heating, cooling, hydro_heating: c_loc of an array of ncell, or c_null_ptr
     integer(c_int) function ftte_thermal_equilibrium(ctx, run_uvb_transfer, J, gamma, uniform_gamma, self_shielding_threshold, &
          use_point_rates, heating, cooling, hydro_heating) bind(C, name='ftte_thermal_equilibrium')
       import :: c_ptr, c_int, c_double
       type(c_ptr), value :: ctx
       integer(c_int), value :: run_uvb_transfer, use_point_rates
       real(c_double), intent(in) :: J(*)          ! (ncell, 3): Jmean1..3
       real(c_double), intent(in) :: gamma(3,3)    ! (gammaHI, gammaHeI, gammaHeII) x (group1, group2, group3)
       real(c_double), intent(in) :: uniform_gamma(3) ! the uniform background's gammas of HI, HeII, HeI
       real(c_double), value :: self_shielding_threshold
       type(c_ptr), value :: heating, cooling, hydro_heating
     end function ftte_thermal_equilibrium

     integer(c_int) function ftte_thermal_equilibrium_device(ctx, run_uvb_transfer, J_dev, gamma, uniform_gamma, &
          self_shielding_threshold, use_point_rates, heating, cooling, hydro_heating) bind(C, name='ftte_thermal_equilibrium_device')
       import :: c_ptr, c_int, c_double
       type(c_ptr), value :: ctx
       integer(c_int), value :: run_uvb_transfer, use_point_rates
       type(c_ptr), value :: J_dev
       real(c_double), intent(in) :: gamma(3,3)
       real(c_double), intent(in) :: uniform_gamma(3)
       real(c_double), value :: self_shielding_threshold
       type(c_ptr), value :: heating, cooling, hydro_heating
     end function ftte_thermal_equilibrium_device

     ! the temperature advanced over dt_s seconds in `substeps` implicit steps at fixed species, clipped to [tmin, tmax];
     ! use_hydro_heating adds the hydroHeating of the last ftte_thermal_equilibrium; the rate arguments as there
     integer(c_int) function ftte_advance_temperature(ctx, dt_s, substeps, tmin, tmax, use_hydro_heating, run_uvb_transfer, J, gamma, &
          uniform_gamma, self_shielding_threshold, use_point_rates, max_change) bind(C, name='ftte_advance_temperature')
       import :: c_ptr, c_int, c_double
       type(c_ptr), value :: ctx
       real(c_double), value :: dt_s, tmin, tmax
       integer(c_int), value :: substeps, use_hydro_heating, run_uvb_transfer, use_point_rates
       real(c_double), intent(in) :: J(*)
       real(c_double), intent(in) :: gamma(3,3)
       real(c_double), intent(in) :: uniform_gamma(3)
       real(c_double), value :: self_shielding_threshold
       real(c_double), intent(out) :: max_change
     end function ftte_advance_temperature

     integer(c_int) function ftte_advance_temperature_device(ctx, dt_s, substeps, tmin, tmax, use_hydro_heating, run_uvb_transfer, &
          J_dev, gamma, uniform_gamma, self_shielding_threshold, use_point_rates, max_change) &
          bind(C, name='ftte_advance_temperature_device')
       import :: c_ptr, c_int, c_double
       type(c_ptr), value :: ctx
       real(c_double), value :: dt_s, tmin, tmax
       integer(c_int), value :: substeps, use_hydro_heating, run_uvb_transfer, use_point_rates
       type(c_ptr), value :: J_dev
       real(c_double), intent(in) :: gamma(3,3)
       real(c_double), intent(in) :: uniform_gamma(3)
       real(c_double), value :: self_shielding_threshold
       real(c_double), intent(out) :: max_change
     end function ftte_advance_temperature_device

     ! species and temperature of every leaf advanced together over dt_s seconds, each leaf in at most max_subcycles subcycles of
     ! h = min(remaining, max(eta tau, remaining/(max_subcycles - s))), tau its own time scale; ksi, uniform as
     ! ftte_advance_rate_equations takes them, gamma, uniform_gamma as ftte_advance_temperature does.  max_change: the largest change
     ! of a species fraction and of T; subcycles: their sum, the largest count of a leaf, the leaves the cap bounded
     integer(c_int) function ftte_advance_thermochemistry(ctx, dt_s, eta, max_subcycles, tmin, tmax, use_hydro_heating, &
          run_uvb_transfer, J, ksi, gamma, uniform, uniform_gamma, self_shielding_threshold, use_point_rates, max_change, subcycles) &
          bind(C, name='ftte_advance_thermochemistry')
       import :: c_ptr, c_int, c_double, c_int64_t
       type(c_ptr), value :: ctx
       real(c_double), value :: dt_s, eta, tmin, tmax
       integer(c_int), value :: max_subcycles, use_hydro_heating, run_uvb_transfer, use_point_rates
       real(c_double), intent(in) :: J(*)          ! (ncell, 3): Jmean1..3
       real(c_double), intent(in) :: ksi(3,3)      ! (ksi24, ksi25, ksi26) x (group1, group2, group3)
       real(c_double), intent(in) :: gamma(3,3)    ! (gammaHI, gammaHeI, gammaHeII) x (group1, group2, group3)
       real(c_double), intent(in) :: uniform(3)
       real(c_double), intent(in) :: uniform_gamma(3)
       real(c_double), value :: self_shielding_threshold
       real(c_double), intent(out) :: max_change(2)
       integer(c_int64_t), intent(out) :: subcycles(3)
     end function ftte_advance_thermochemistry

     integer(c_int) function ftte_advance_thermochemistry_device(ctx, dt_s, eta, max_subcycles, tmin, tmax, use_hydro_heating, &
          run_uvb_transfer, J_dev, ksi, gamma, uniform, uniform_gamma, self_shielding_threshold, use_point_rates, max_change, &
          subcycles) bind(C, name='ftte_advance_thermochemistry_device')
       import :: c_ptr, c_int, c_double, c_int64_t
       type(c_ptr), value :: ctx
       real(c_double), value :: dt_s, eta, tmin, tmax
       integer(c_int), value :: max_subcycles, use_hydro_heating, run_uvb_transfer, use_point_rates
       type(c_ptr), value :: J_dev
       real(c_double), intent(in) :: ksi(3,3)
       real(c_double), intent(in) :: gamma(3,3)
       real(c_double), intent(in) :: uniform(3)
       real(c_double), intent(in) :: uniform_gamma(3)
       real(c_double), value :: self_shielding_threshold
       real(c_double), intent(out) :: max_change(2)
       integer(c_int64_t), intent(out) :: subcycles(3)
     end function ftte_advance_thermochemistry_device

     ! the subcycles each leaf took in the last such call
     integer(c_int) function ftte_get_subcycles(ctx, per_leaf) bind(C, name='ftte_get_subcycles')
       import :: c_ptr, c_int, c_int32_t
       type(c_ptr), value :: ctx
       integer(c_int32_t), intent(out) :: per_leaf(*) ! (ncell)
     end function ftte_get_subcycles

     ! ---- diffuse recombination radiation (the build's own; include/ftte.h) -----------------------------------------------------
     ! g(nratec, 3): the coefficients of recombination to the ground states of HI, HeI, HeII on the rate coefficients' temperature grid
     integer(c_int) function ftte_set_ground_recombination(ctx, nratec, g) bind(C, name='ftte_set_ground_recombination')
       import :: c_ptr, c_int, c_double
       type(c_ptr), value :: ctx
       integer(c_int), value :: nratec
       real(c_double), intent(in) :: g(*)          ! (nratec, 3)
     end function ftte_set_ground_recombination

     ! the source function of every leaf from the device-resident gas state, into the context's emission field: the next sweep
     ! carries it.  S: c_loc of a host array (ncell, 3), or c_null_ptr; lost: c_loc of an integer(c_int64_t), or c_null_ptr
     integer(c_int) function ftte_recombination_source(ctx, ksi, share, S, lost) bind(C, name='ftte_recombination_source')
       import :: c_ptr, c_int, c_double
       type(c_ptr), value :: ctx
       real(c_double), intent(in) :: ksi(3,3)      ! (ksi24, ksi25, ksi26) x (group1, group2, group3)
       real(c_double), intent(in) :: share(3,3)    ! (group1, group2, group3) x (HII, HeII, HeIII recombining)
       type(c_ptr), value :: S
       type(c_ptr), value :: lost
     end function ftte_recombination_source

     integer(c_int) function ftte_recombination_source_device(ctx, ksi, share, S_dev, lost) &
          bind(C, name='ftte_recombination_source_device')
       import :: c_ptr, c_int, c_double
       type(c_ptr), value :: ctx
       real(c_double), intent(in) :: ksi(3,3)
       real(c_double), intent(in) :: share(3,3)
       type(c_ptr), value :: S_dev
       type(c_ptr), value :: lost
     end function ftte_recombination_source_device

  end interface

contains

  ! the reference's error convention: print and stop (e.g. equiSources.f90:1412, transportRoutinesModule.f90:33-36)
  subroutine ftteCheck(ctx, status, where)
    type(c_ptr), intent(in) :: ctx
    integer(c_int), intent(in) :: status
    character(len=*), intent(in) :: where
    character(kind=c_char), pointer :: msg(:)
    type(c_ptr) :: p
    integer :: n
    if (status == FTTE_OK) return
    p = ftte_last_error(ctx)
    if (c_associated(p)) then
       call c_f_pointer(p, msg, [1024])
       n = 0
       do while (n < 1024)
          if (msg(n+1) == c_null_char) exit
          n = n + 1
       enddo
       write(*,*) 'ftte error in ', where, ': status', status, ' ', msg(1:n)
    else
       write(*,*) 'ftte error in ', where, ': status', status
    endif
    stop 1
  end subroutine ftteCheck

end module ftte_binding
