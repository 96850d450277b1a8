! ftte_rate_equations.f90 -- the drop-ins for the chemistry: what replaces the start-up equilibrium equiSources.f90:1008-1022,
! the solveRateEquations calls of the loop :1824-1831 and the loop's computeMass calls in the reference driver.
!
! Compiled TOGETHER WITH the reference (module `definitions`); this repository compiles it only as an interface check
! against oracle/_ref/definitions.mod (fortran/Makefile: target `dropin-check`).
!
!   call ftteInitialIonizationEquilibrium(nx)        ! replaces :1008-1022 (both passes, computeMass, the printed fraction)
!   call ftteThermalEquilibrium(nx)                  ! replaces :1025-1033 (thermalEquilibrium for every leaf; sets hydroHeating)
!   call ftteExpandHIIRegions(nx, nStars, star)      ! replaces :1035-1069, inside `if (expansionFlag)` (off in the shipped source)
!   call ftteSolveRateEquations(nx, runUVBTransfer)  ! replaces the solveRateEquations calls of :1824-1831
!   call ftteComputeMass(nx)                         ! replaces the computeMass calls of :1824-1831
!
! On entry the leaves hold rho, tgas, HI, HeI, HeII, krate24..26 (the point-source block) and Jmean1..3 (the diffuse
! block); on return HI, HeI, HeII are the reference's new equilibrium values.  ftteInitialIonizationEquilibrium and
! ftteComputeMass set neutralHydrogenMass and totalHydrogenMass.  ftteExpandHIIRegions works on the medium the start-up
! equilibrium left on the device (before it has run it takes the tree) and leaves rhoCoef, rho, HI, HeI, HeII of every leaf as the
! reference's findExpansion and applyExpansion do.  ftteComputeMass works on the medium the last of the
! other two left on the device (the tree's HI and rho unchanged since); before either has run it takes the tree.
module ftte_rate_equations

  use, intrinsic :: iso_c_binding
  use definitions
  use ftte_binding
  implicit none

  type(c_ptr), save, private :: ctx = c_null_ptr
  integer(c_int64_t), private :: cursor
  logical, save, private :: resident = .false.   ! the context's medium is the tree's

contains

  subroutine ftteSolveRateEquations(nx, runUVBTransfer)
    integer, intent(in) :: nx
    logical, intent(in) :: runUVBTransfer
    integer(c_int64_t) :: ncell
    integer(c_int32_t), allocatable :: lev(:)
    real(c_double), allocatable :: f(:,:), rates(:,:)
    real(c_double) :: ksi(3,3), uniform(3), change
    integer(c_int) :: uvb
    integer :: i, j, k

    if (.not. c_associated(ctx)) call ftteCheck(c_null_ptr, ftte_create(ctx, 1, c_null_ptr), 'ftte_create')

    ncell = 0
    do i = 1, nx
       do j = 1, nx
          do k = 1, nx
             call countChemCells(baseGrid%cell(i,j,k), ncell)
          enddo
       enddo
    enddo
    allocate(lev(ncell), f(ncell,11), rates(ncell,6))
    cursor = 0
    do i = 1, nx
       do j = 1, nx
          do k = 1, nx
             call gatherState(baseGrid%cell(i,j,k), 0, lev, f)
          enddo
       enddo
    enddo
    rates = 0.d0
    rates(:,1:3) = f(:,6:8)

    ksi(:,1) = (/ group1%ksi24, group1%ksi25, group1%ksi26 /)
    ksi(:,2) = (/ group2%ksi24, group2%ksi25, group2%ksi26 /)
    ksi(:,3) = (/ group3%ksi24, group3%ksi25, group3%ksi26 /)
    uniform = (/ uniformQuasar*quasar%ksi24 + uniformStellar*stellar%ksi24, &
                 uniformQuasar*quasar%ksi25 + uniformStellar*stellar%ksi25, &
                 uniformQuasar*quasar%ksi26 + uniformStellar*stellar%ksi26 /)
    uvb = 0
    if (runUVBTransfer) uvb = 1

    call ftteCheck(ctx, ftte_set_grid(ctx, nx, nx, nx, ncell, lev, physicalBoxSize), 'ftte_set_grid')
    call ftteCheck(ctx, ftte_set_rate_coefficients(ctx, nratec, logtem0, logtem9, dlogtem, k1a, k2a, k3a, k4a, k5a, k6a), &
         'ftte_set_rate_coefficients')
    call ftteCheck(ctx, ftte_set_medium(ctx, f(:,3), f(:,4), f(:,5), f(:,1), f(:,1), 0), 'ftte_set_medium')
    call ftteCheck(ctx, ftte_set_temperature(ctx, f(:,2)), 'ftte_set_temperature')
    call ftteCheck(ctx, ftte_set_point_rates(ctx, rates), 'ftte_set_point_rates')
    call ftteCheck(ctx, ftte_solve_rate_equations(ctx, uvb, f(:,9:11), ksi, uniform, selfShieldingThreshold, 1, change), &
         'ftte_solve_rate_equations')
    call ftteCheck(ctx, ftte_get_medium(ctx, f(:,3), f(:,4), f(:,5)), 'ftte_get_medium')

    cursor = 0
    do i = 1, nx
       do j = 1, nx
          do k = 1, nx
             call scatterState(baseGrid%cell(i,j,k), f)
          enddo
       enddo
    enddo
    resident = .true.
  end subroutine ftteSolveRateEquations

  ! the tree's leaves -> the context: grid, rate coefficients, medium with rho, temperature; f(ncell,11) as gatherState fills it
  subroutine loadTree(nx, f)
    integer, intent(in) :: nx
    real(c_double), allocatable, intent(out) :: f(:,:)
    integer(c_int64_t) :: ncell
    integer(c_int32_t), allocatable :: lev(:)
    integer :: i, j, k

    if (.not. c_associated(ctx)) call ftteCheck(c_null_ptr, ftte_create(ctx, 1, c_null_ptr), 'ftte_create')
    ncell = 0
    do i = 1, nx
       do j = 1, nx
          do k = 1, nx
             call countChemCells(baseGrid%cell(i,j,k), ncell)
          enddo
       enddo
    enddo
    allocate(lev(ncell), f(ncell,11))
    cursor = 0
    do i = 1, nx
       do j = 1, nx
          do k = 1, nx
             call gatherState(baseGrid%cell(i,j,k), 0, lev, f)
          enddo
       enddo
    enddo
    call ftteCheck(ctx, ftte_set_grid(ctx, nx, nx, nx, ncell, lev, physicalBoxSize), 'ftte_set_grid')
    call ftteCheck(ctx, ftte_set_rate_coefficients(ctx, nratec, logtem0, logtem9, dlogtem, k1a, k2a, k3a, k4a, k5a, k6a), &
         'ftte_set_rate_coefficients')
    call ftteCheck(ctx, ftte_set_medium(ctx, f(:,3), f(:,4), f(:,5), f(:,1), f(:,1), 0), 'ftte_set_medium')
    call ftteCheck(ctx, ftte_set_temperature(ctx, f(:,2)), 'ftte_set_temperature')
  end subroutine loadTree

  ! equiSources.f90:1008-1022: initialIonizationEquilibrium twice for every leaf, computeMass, the printed neutral fraction
  subroutine ftteInitialIonizationEquilibrium(nx)
    integer, intent(in) :: nx
    real(c_double), allocatable :: f(:,:)
    real(c_double) :: uniform(3), fraction
    integer :: i, j, k

    print*, 'computing ionization equilibrium'
    call loadTree(nx, f)
    uniform = (/ uniformQuasar*quasar%ksi24 + uniformStellar*stellar%ksi24, &
                 uniformQuasar*quasar%ksi25 + uniformStellar*stellar%ksi25, &
                 uniformQuasar*quasar%ksi26 + uniformStellar*stellar%ksi26 /)
    call ftteCheck(ctx, ftte_initial_ionization_equilibrium(ctx, uniform, selfShieldingThreshold, 2, fraction), &
         'ftte_initial_ionization_equilibrium')
    call ftteCheck(ctx, ftte_get_medium(ctx, f(:,3), f(:,4), f(:,5)), 'ftte_get_medium')
    cursor = 0
    do i = 1, nx
       do j = 1, nx
          do k = 1, nx
             call scatterState(baseGrid%cell(i,j,k), f)
          enddo
       enddo
    enddo
    resident = .true.
    call ftteCheck(ctx, ftte_hydrogen_mass(ctx, neutralHydrogenMass, totalHydrogenMass), 'ftte_hydrogen_mass')
    write(*,'("ionization equilibrium:", es18.8)') neutralHydrogenMass/totalHydrogenMass
  end subroutine ftteInitialIonizationEquilibrium

  ! equiSources.f90:1035-1069: the density drop of the HII regions around every star with weight > 0.  The device computes
  ! rhoCoef and scales its own medium; the tree takes rhoCoef and the reference's own applyExpansion rule (:4495-4500), the same
  ! four multiplications, so its fields equal the device's bit for bit.
  subroutine ftteExpandHIIRegions(nx, nStars, star)
    integer, intent(in) :: nx, nStars
    type(starType), intent(in) :: star(:)
    real(c_double), allocatable :: f(:,:), coef(:)
    integer(c_int64_t), allocatable :: host(:)
    integer(c_int32_t), allocatable :: pos(:)
    integer(c_int64_t) :: ncell, nchanged
    integer(c_int) :: nsrc
    integer :: i, j, k, iStar

    print*, 'computing expansion of HII regions'
    if (.not. resident) then
       call loadTree(nx, f)
       resident = .true.
    endif
    ncell = 0
    do i = 1, nx
       do j = 1, nx
          do k = 1, nx
             call countChemCells(baseGrid%cell(i,j,k), ncell)
          enddo
       enddo
    enddo
    allocate(host(max(nStars,1)), coef(ncell))
    nsrc = 0
    do iStar = 1, nStars
       if (star(iStar)%weight .gt. 0) then
          allocate(pos(3*star(iStar)%level+3))
          pos = star(iStar)%position(1:3*star(iStar)%level+3)
          nsrc = nsrc + 1
          call ftteCheck(ctx, ftte_locate_cell(ctx, star(iStar)%level, pos, host(nsrc)), 'ftte_locate_cell')
          deallocate(pos)
       endif
    enddo
    call ftteCheck(ctx, ftte_expand_hii_regions(ctx, nsrc, host, c_null_ptr, coef, nchanged), 'ftte_expand_hii_regions')
    cursor = 0
    do i = 1, nx
       do j = 1, nx
          do k = 1, nx
             call scatterExpansion(baseGrid%cell(i,j,k), coef)
          enddo
       enddo
    enddo
  end subroutine ftteExpandHIIRegions

  ! rhoCoef into the tree, then applyExpansion's rule (equiSources.f90:4495-4500)
  recursive subroutine scatterExpansion(c, coef)
    type(zoneType) :: c
    real(c_double), intent(in) :: coef(:)
    integer :: a, b, d
    if (c%refined) then
       do a = 1, 2
          do b = 1, 2
             do d = 1, 2
                call scatterExpansion(c%cell(a,b,d), coef)
             enddo
          enddo
       enddo
    else
       cursor = cursor + 1
       c%rhoCoef = coef(cursor)
       if (c%rhoCoef.lt.1.) then
          c%rho  = c%rho  * c%rhoCoef
          c%HI   = c%HI   * c%rhoCoef
          c%HeI  = c%HeI  * c%rhoCoef
          c%HeII = c%HeII * c%rhoCoef
       endif
    endif
  end subroutine scatterExpansion

  ! computeMass (equiSources.f90:4369-4393) over every leaf: neutralHydrogenMass, totalHydrogenMass [msun]
  subroutine ftteComputeMass(nx)
    integer, intent(in) :: nx
    real(c_double), allocatable :: f(:,:)

    if (.not. resident) then
       call loadTree(nx, f)
       resident = .true.
    endif
    call ftteCheck(ctx, ftte_hydrogen_mass(ctx, neutralHydrogenMass, totalHydrogenMass), 'ftte_hydrogen_mass')
  end subroutine ftteComputeMass

  ! equiSources.f90:1025-1033: thermalEquilibrium for every leaf, from the module's own cooling tables as calc_rates filled them.
  ! hydroHeating goes back into the tree and stays on the device, where ftte_advance_temperature adds it behind its flag.
  subroutine ftteThermalEquilibrium(nx)
    integer, intent(in) :: nx
    real(c_double), allocatable :: f(:,:), cool(:,:)
    real(c_double), allocatable, target :: hydro(:)
    real(c_double) :: gamma(3,3), uniformGamma(3)
    integer :: i, j, k

    call loadTree(nx, f)
    resident = .true.
    allocate(cool(nratec,13), hydro(size(f,1)))
    cool(:,1) = ceHIa;   cool(:,2) = ceHeIa;   cool(:,3) = ceHeIIa;   cool(:,4) = ciHIa;     cool(:,5) = ciHeIa
    cool(:,6) = ciHeISa; cool(:,7) = ciHeIIa;  cool(:,8) = reHIIa;    cool(:,9) = reHeII1a;  cool(:,10) = reHeII2a
    cool(:,11) = reHeIIIa; cool(:,12) = brema; cool(:,13) = lineHIa
    call ftteCheck(ctx, ftte_set_cooling_coefficients(ctx, nratec, cool, compa, currentRedshift), 'ftte_set_cooling_coefficients')
    gamma = 0.d0
    uniformGamma = (/ uniformQuasar*quasar%gammaHI + uniformStellar*stellar%gammaHI, &
                      uniformQuasar*quasar%gammaHeII + uniformStellar*stellar%gammaHeII, &
                      uniformQuasar*quasar%gammaHeI + uniformStellar*stellar%gammaHeI /)
    call ftteCheck(ctx, ftte_thermal_equilibrium(ctx, 0, f(:,9:11), gamma, uniformGamma, selfShieldingThreshold, 0, c_null_ptr, &
         c_null_ptr, c_loc(hydro)), 'ftte_thermal_equilibrium')
    cursor = 0
    do i = 1, nx
       do j = 1, nx
          do k = 1, nx
             call scatterHydroHeating(baseGrid%cell(i,j,k), hydro)
          enddo
       enddo
    enddo
  end subroutine ftteThermalEquilibrium

  recursive subroutine scatterHydroHeating(c, hydro)
    type(zoneType) :: c
    real(c_double), intent(in) :: hydro(:)
    integer :: a, b, d
    if (c%refined) then
       do a = 1, 2
          do b = 1, 2
             do d = 1, 2
                call scatterHydroHeating(c%cell(a,b,d), hydro)
             enddo
          enddo
       enddo
    else
       cursor = cursor + 1
       c%hydroHeating = hydro(cursor)
    endif
  end subroutine scatterHydroHeating

  recursive subroutine countChemCells(c, total)
    type(zoneType) :: c
    integer(c_int64_t), intent(inout) :: total
    integer :: a, b, d
    if (c%refined) then
       do a = 1, 2
          do b = 1, 2
             do d = 1, 2
                call countChemCells(c%cell(a,b,d), total)
             enddo
          enddo
       enddo
    else
       total = total + 1
    endif
  end subroutine countChemCells

  recursive subroutine gatherState(c, level, lev, f)
    type(zoneType) :: c
    integer, intent(in) :: level
    integer(c_int32_t), intent(inout) :: lev(:)
    real(c_double), intent(inout) :: f(:,:)
    integer :: a, b, d
    if (c%refined) then
       do a = 1, 2
          do b = 1, 2
             do d = 1, 2
                call gatherState(c%cell(a,b,d), level+1, lev, f)
             enddo
          enddo
       enddo
    else
       cursor = cursor + 1
       lev(cursor) = level
       f(cursor,1) = c%rho
       f(cursor,2) = c%tgas
       f(cursor,3) = c%HI
       f(cursor,4) = c%HeI
       f(cursor,5) = c%HeII
       f(cursor,6) = c%krate24
       f(cursor,7) = c%krate25
       f(cursor,8) = c%krate26
       f(cursor,9) = c%Jmean1
       f(cursor,10) = c%Jmean2
       f(cursor,11) = c%Jmean3
    endif
  end subroutine gatherState

  recursive subroutine scatterState(c, f)
    type(zoneType) :: c
    real(c_double), intent(in) :: f(:,:)
    integer :: a, b, d
    if (c%refined) then
       do a = 1, 2
          do b = 1, 2
             do d = 1, 2
                call scatterState(c%cell(a,b,d), f)
             enddo
          enddo
       enddo
    else
       cursor = cursor + 1
       c%HI = f(cursor,3)
       c%HeI = f(cursor,4)
       c%HeII = f(cursor,5)
    endif
  end subroutine scatterState

end module ftte_rate_equations
