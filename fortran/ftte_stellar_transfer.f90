! ftte_stellar_transfer.f90 -- the drop-in for the point-source block: what replaces the star loop
! equiSources.f90:1260-1362 inside `if (runStellarTransfer)` in the reference driver, its per-star `src:` line (escape fractions
! at the seven output radii, :1342-1357) and the accumulation of cosmicSpectrum (:1350-1351) included.
!
! Compiled TOGETHER WITH the reference (modules `definitions` and `dust`); this repository compiles it only as an
! interface check against oracle/_ref/*.mod (fortran/Makefile: target `dropin-check`).
!
!   call setZeroRates(...)                                   ! unchanged, the reference zeroes the cells itself
!   call ftteRunStellarTransfer(nx, nStars, star, iSpectrum, coefSpectrum)
!
! On return krate24..26 and crate24..26 of every leaf hold what the reference's startNewLongRay deposits, highestPixelLevel and
! (per star, as after the reference's loop the last star's) ndotRemaining, ndotBoundary, ndotDust, ndotSpectrum, fraction of
! module localDefinitions / definitions are set, and cosmicSpectrum has received every star's share; the caller zeroes
! cosmicSpectrum before (:1258) and divides by nStarsSpecificAge after (:1366), as the reference does around its loop.
! localDefinitions is a module of the reference's main file: compile this file after it (INTEGRATION.md).
!
! In front of it, where the stars come as coordinates: call ftteStarCatalogue(nx, nStars, xyz, lo, hi, star) replaces :750-757 of
! the ingest loop and the whole of :1169-1212 (host leaves, call sequences, stars of one leaf merged); see there.
!
! ftteStarBatch (default 1: the reference's sequence, one table build and one trace per star).  Set it larger and that many stars
! are traced together: each star's (iMetal, coefMetal) as before, stars with identical pairs share a population slot, one
! ftte_stellar_beta_tables and one ftte_point_sources_populations per batch; the per-star results follow in star order.
! The environment variable FTTE_STAR_BATCH sets it without a recompilation.  It is read once, at the module's first call, and where
! it holds a number >= 1 it wins over a value the host program assigned before that call; a value assigned after the first call
! holds from the next call on.
module ftte_stellar_transfer

  use, intrinsic :: iso_c_binding
  use definitions
  use localDefinitions
  use dust
  use ftte_binding
  implicit none

  integer, save, public :: ftteStarBatch = 1
  type(c_ptr), save, private :: ctx = c_null_ptr
  integer(c_int64_t), private :: cursor

contains

  subroutine ftteRunStellarTransfer(nx, nStars, star, iSpectrum, coefSpectrum)
    integer, intent(in) :: nx, nStars, iSpectrum
    type(starType), intent(in) :: star(:)
    real(kind=RealKind), intent(in) :: coefSpectrum
    integer(c_int64_t) :: ncell, host(1)
    integer(c_int32_t), allocatable :: lev(:), pos(:)
    real(c_double), allocatable :: med(:,:), rates(:,:)
    real(c_double) :: ndot(1), totalIntegral, tmp, coefMetal
    real(c_double) :: escRemaining(nradius), escBoundary(nradius), escDust(1), escSpectrum(nenergy), escFraction(nradius)
    integer(c_int) :: highest
    integer :: i, j, k, iStar, iMetal
    ! a batch of stars (ftteStarBatch > 1) and its populations
    integer(c_int64_t), allocatable :: bHost(:)
    real(c_double), allocatable :: bNdot(:), popCoefS(:), popCoefM(:), popTotal(:)
    real(c_double), allocatable :: bRemaining(:,:), bBoundary(:,:), bDust(:), bSpectrum(:,:), bFraction(:,:)
    integer(c_int32_t), allocatable :: bSlot(:)
    integer(c_int), allocatable :: bHighest(:), popSpectrum(:), popMetal(:)
    integer, allocatable :: bStar(:)
    integer :: nb, npop, ip, ib, nbatch, envStatus, envValue
    character(len=16) :: envText

    if (.not. c_associated(ctx)) then
       call ftteCheck(c_null_ptr, ftte_create(ctx, 1, c_null_ptr), 'ftte_create')
       call get_environment_variable('FTTE_STAR_BATCH', envText, status=envStatus)
       if (envStatus .eq. 0) then
          read(envText, *, iostat=envStatus) envValue
          if (envStatus .eq. 0 .and. envValue .ge. 1) ftteStarBatch = envValue
       endif
    endif

    ncell = 0
    do i = 1, nx
       do j = 1, nx
          do k = 1, nx
             call countCells(baseGrid%cell(i,j,k), ncell)
          enddo
       enddo
    enddo
    allocate(lev(ncell), med(ncell,5), rates(ncell,6))
    cursor = 0
    do i = 1, nx
       do j = 1, nx
          do k = 1, nx
             call gatherMedium(baseGrid%cell(i,j,k), 0, lev, med)
          enddo
       enddo
    enddo

    call ftteCheck(ctx, ftte_set_grid(ctx, nx, nx, nx, ncell, lev, physicalBoxSize), 'ftte_set_grid')
    call ftteCheck(ctx, ftte_set_medium(ctx, med(:,1), med(:,2), med(:,3), med(:,4), med(:,5), dustApproximation), &
         'ftte_set_medium')
    call ftteCheck(ctx, ftte_set_zero_rates(ctx), 'ftte_set_zero_rates')

    nbatch = max(1, min(ftteStarBatch, nStars))
    if (nbatch .gt. 1) then
       allocate(bHost(nbatch), bNdot(nbatch), bSlot(nbatch), bHighest(nbatch), bStar(nbatch))
       allocate(popSpectrum(nbatch), popCoefS(nbatch), popMetal(nbatch), popCoefM(nbatch), popTotal(nbatch))
       allocate(bRemaining(nradius,nbatch), bBoundary(nradius,nbatch), bDust(nbatch), bSpectrum(nenergy,nbatch), &
            bFraction(nradius,nbatch))
    endif
    nb = 0
    npop = 0

    do iStar = 1, nStars
       if (star(iStar)%weight .gt. 0) then
          allocate(pos(3*star(iStar)%level+3))
          pos = star(iStar)%position(1:3*star(iStar)%level+3)
          call ftteCheck(ctx, ftte_locate_cell(ctx, star(iStar)%level, pos, host(1)), 'ftte_locate_cell')
          deallocate(pos)

          ! the population of this star: metallicity of its host cell, equiSources.f90:1281-1291
          if (med(host(1)+1,5) .gt. 1.e-20) then
             tmp = dlog10(med(host(1)+1,5))
          else
             tmp = - 20.
          endif
          iMetal = 1
          do while (tmp .gt. metallicity(iMetal+1))
             iMetal = iMetal + 1
             if (iMetal+1 .eq. nMetallicity) exit
          enddo
          coefMetal = (tmp-metallicity(iMetal))/(metallicity(iMetal+1)-metallicity(iMetal))
          coefMetal = min(max(0.d0,coefMetal),1.d0)

          if (nbatch .gt. 1) then
             ! into the batch: the slot of this star's population, a new one unless an earlier star of the batch has the same pair
             ip = 1
             do while (ip .le. npop)
                if (popMetal(ip) .eq. iMetal .and. popCoefM(ip) .eq. coefMetal) exit
                ip = ip + 1
             enddo
             if (ip .gt. npop) then
                npop = ip
                popSpectrum(ip) = iSpectrum
                popCoefS(ip) = coefSpectrum
                popMetal(ip) = iMetal
                popCoefM(ip) = coefMetal
             endif
             nb = nb + 1
             bStar(nb) = iStar
             bHost(nb) = host(1)
             bNdot(nb) = float(star(iStar)%weight)
             bSlot(nb) = ip - 1
             if (nb .eq. nbatch) call traceBatch
             cycle
          endif

          call ftteCheck(ctx, ftte_stellar_beta_table(ctx, a_smc, nWavelengths, wavelength, nSpectra, nMetallicity, &
               specificLuminosity, iSpectrum, coefSpectrum, iMetal, coefMetal, totalIntegral), 'ftte_stellar_beta_table')

          ndot(1) = float(star(iStar)%weight)       ! :1303
          call ftteCheck(ctx, ftte_point_sources(ctx, 1, host, ndot, highest), 'ftte_point_sources')
          highestPixelLevel = highest

          ! what the tracer kept for this star (:3198-3233, :3336-3345), the src: line (:1342-1357) and the cosmic spectrum
          call ftteCheck(ctx, ftte_point_escape(ctx, 1, escRemaining, escBoundary, escDust, escSpectrum, escFraction), 'ftte_point_escape')
          ndotRemaining = escRemaining
          ndotBoundary = escBoundary
          ndotDust = escDust(1)
          ndotSpectrum = escSpectrum
          fraction = escFraction
          cosmicSpectrum = cosmicSpectrum + float(star(iStar)%weight) * ndotSpectrum/(ndot(1)-ndotBoundary(nradius))
          write(*,1015) iStar, star(iStar)%level, med(host(1)+1,1) * mh / (psi * med(host(1)+1,4)), &
               highestPixelLevel, fraction, star(iStar)%weight
1015      format('src: ', i5, i3, es13.5, i3, 7f9.5, i8)
       endif
    enddo
    if (nb .gt. 0) call traceBatch

    call ftteCheck(ctx, ftte_get_point_rates(ctx, rates), 'ftte_get_point_rates')
    cursor = 0
    do i = 1, nx
       do j = 1, nx
          do k = 1, nx
             call scatterRates(baseGrid%cell(i,j,k), rates)
          enddo
       enddo
    enddo

  contains

    ! the nb stars collected so far: their npop populations in one call, the stars in one call, then per star and in star order
    ! what the loop above produces for a single star
    subroutine traceBatch
      call ftteCheck(ctx, ftte_stellar_beta_tables(ctx, a_smc, nWavelengths, wavelength, nSpectra, nMetallicity, &
           specificLuminosity, npop, popSpectrum, popCoefS, popMetal, popCoefM, popTotal), 'ftte_stellar_beta_tables')
      call ftteCheck(ctx, ftte_point_sources_populations(ctx, nb, bHost, bNdot, bSlot, bHighest), &
           'ftte_point_sources_populations')
      call ftteCheck(ctx, ftte_point_escape(ctx, nb, bRemaining, bBoundary, bDust, bSpectrum, bFraction), 'ftte_point_escape')
      do ib = 1, nb
         highestPixelLevel = bHighest(ib)
         ndotRemaining = bRemaining(:,ib)
         ndotBoundary = bBoundary(:,ib)
         ndotDust = bDust(ib)
         ndotSpectrum = bSpectrum(:,ib)
         fraction = bFraction(:,ib)
         cosmicSpectrum = cosmicSpectrum + float(star(bStar(ib))%weight) * ndotSpectrum/(bNdot(ib)-ndotBoundary(nradius))
         write(*,1016) bStar(ib), star(bStar(ib))%level, med(bHost(ib)+1,1) * mh / (psi * med(bHost(ib)+1,4)), &
              highestPixelLevel, fraction, star(bStar(ib))%weight
1016     format('src: ', i5, i3, es13.5, i3, 7f9.5, i8)
      enddo
      nb = 0
      npop = 0
    end subroutine traceBatch

  end subroutine ftteRunStellarTransfer

  ! What replaces equiSources.f90:750-757 for every star and the whole of :1169-1212: the stars' coordinates xyz(3,nStars) in the
  ! units of the box corners lo, hi (the reference's xa..zb); on entry star(:)%weight holds what the age filter (:773-783) gave.
  ! On return star(:)%level and %position are the host leaf's (allocated here), and %weight is the sum over the stars of the
  ! leaf on the leaf's first star with weight > 0 and 0 on the others, so that the rest of the driver and ftteRunStellarTransfer
  ! run on the result.  Stars are merged by host leaf, not by the reference's location key (include/ftte.h).  A star outside the
  ! box gets weight 0, level 0 and position (0,0,0); nOutside (optional) counts them.
  subroutine ftteStarCatalogue(nx, nStars, xyz, lo, hi, star, nOutside)
    integer, intent(in) :: nx, nStars
    real(kind=RealKind), intent(in) :: xyz(3,nStars), lo(3), hi(3)
    type(starType), intent(inout) :: star(:)
    integer, intent(out), optional :: nOutside
    integer(c_int64_t) :: ncell, nsrc, outside
    integer(c_int32_t), allocatable, target :: lev(:), w(:), srcWeight(:)
    integer(c_int64_t), allocatable, target :: cells(:), firstStar(:)
    real(c_double), allocatable :: med(:,:)
    integer(c_int32_t) :: pos(183)
    integer(c_int) :: level
    integer :: i, j, k, iStar

    if (.not. c_associated(ctx)) call ftteCheck(c_null_ptr, ftte_create(ctx, 1, c_null_ptr), 'ftte_create')
    ncell = 0
    do i = 1, nx
       do j = 1, nx
          do k = 1, nx
             call countCells(baseGrid%cell(i,j,k), ncell)
          enddo
       enddo
    enddo
    allocate(lev(ncell), med(ncell,5), w(nStars), cells(nStars))
    cursor = 0
    do i = 1, nx
       do j = 1, nx
          do k = 1, nx
             call gatherMedium(baseGrid%cell(i,j,k), 0, lev, med)
          enddo
       enddo
    enddo
    call ftteCheck(ctx, ftte_set_grid(ctx, nx, nx, nx, ncell, lev, physicalBoxSize), 'ftte_set_grid')
    do iStar = 1, nStars
       w(iStar) = star(iStar)%weight
    enddo
    call ftteCheck(ctx, ftte_star_catalogue(ctx, int(nStars, c_int64_t), xyz, lo, hi, c_loc(w), c_loc(cells), nsrc, outside), &
         'ftte_star_catalogue')
    allocate(srcWeight(max(nsrc,1_c_int64_t)), firstStar(max(nsrc,1_c_int64_t)))
    call ftteCheck(ctx, ftte_star_sources(ctx, nsrc, c_null_ptr, c_loc(srcWeight), c_null_ptr, c_loc(firstStar), c_null_ptr), &
         'ftte_star_sources')
    do iStar = 1, nStars
       star(iStar)%weight = 0
       if (cells(iStar) .ge. 0) then
          call ftteCheck(ctx, ftte_cell_position(ctx, cells(iStar), level, pos), 'ftte_cell_position')
       else
          level = 0
          pos(1:3) = 0
       endif
       star(iStar)%level = level
       allocate(star(iStar)%position(3*level+3))
       star(iStar)%position = pos(1:3*level+3)
    enddo
    do i = 1, int(nsrc)
       star(firstStar(i)+1)%weight = srcWeight(i)
    enddo
    if (present(nOutside)) nOutside = int(outside)
  end subroutine ftteStarCatalogue

  recursive subroutine countCells(c, total)
    type(zoneType) :: c
    integer(c_int64_t), intent(inout) :: total
    integer :: a, b, d
    if (c%refined) then
       do a = 1, 2
          do b = 1, 2
             do d = 1, 2
                call countCells(c%cell(a,b,d), total)
             enddo
          enddo
       enddo
    else
       total = total + 1
    endif
  end subroutine countCells

  recursive subroutine gatherMedium(c, level, lev, med)
    type(zoneType) :: c
    integer, intent(in) :: level
    integer(c_int32_t), intent(inout) :: lev(:)
    real(c_double), intent(inout) :: med(:,:)
    integer :: a, b, d
    if (c%refined) then
       do a = 1, 2
          do b = 1, 2
             do d = 1, 2
                call gatherMedium(c%cell(a,b,d), level+1, lev, med)
             enddo
          enddo
       enddo
    else
       cursor = cursor + 1
       lev(cursor) = level
       med(cursor,1) = c%HI
       med(cursor,2) = c%HeI
       med(cursor,3) = c%HeII
       med(cursor,4) = c%rho
       med(cursor,5) = c%abun2
    endif
  end subroutine gatherMedium

  recursive subroutine scatterRates(c, rates)
    type(zoneType) :: c
    real(c_double), intent(in) :: rates(:,:)
    integer :: a, b, d
    if (c%refined) then
       do a = 1, 2
          do b = 1, 2
             do d = 1, 2
                call scatterRates(c%cell(a,b,d), rates)
             enddo
          enddo
       enddo
    else
       cursor = cursor + 1
       c%krate24 = c%krate24 + rates(cursor,1)
       c%krate25 = c%krate25 + rates(cursor,2)
       c%krate26 = c%krate26 + rates(cursor,3)
       c%crate24 = c%crate24 + rates(cursor,4)
       c%crate25 = c%crate25 + rates(cursor,5)
       c%crate26 = c%crate26 + rates(cursor,6)
    endif
  end subroutine scatterRates

end module ftte_stellar_transfer
