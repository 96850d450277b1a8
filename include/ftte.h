/* ftte.h -- C ABI of the MI355X diffuse radiative-transfer sweep.
 *
 * The reference (razoumov/radiativeTransfer, "FTTE") has no FFI of its own: its hot path
 * is reached through `use transportRoutinesModule` (equiSources.f90:25) and through code
 * inlined in the main program (equiSources.f90:1372-1808), with state in module globals
 * (definitionsModule.f90:55-62,104,182,256).  This header is the seam cut at
 * equiSources.f90:1383-1806: everything between `computeOpacities` and the chemistry.
 * Each entry point names the reference code it stands in for.
 *
 *   in : the cell array (definitionsModule.f90:323-326: depth-first leaf list, `level` per
 *        leaf, k fastest on the base grid), per-leaf opacities kappa_nu (or species densities
 *        + cross-sections), the inflow uvb_nu, a direction list (phi, theta, weight) BEFORE
 *        folding, the box size
 *   out: J_nu per leaf, same order, overwritten (the reference zeroes J in computeOpacities,
 *        equiSources.f90:4964-4966, then accumulates one term per direction,
 *        transportRoutinesModule.f90:953-955)
 *
 * Conventions: plain C types, caller owns every host array, the library owns its device
 * buffers, every function returns 0 on success or a negative ftte_status (it never calls
 * exit: where the reference executes `stop`, the status says which `stop`).  All arithmetic
 * is IEEE binary64.  A context is not thread-safe; use one per host thread / per GPU.
 *
 * The library is linked against the HIP runtime and needs a gfx950 device for every call
 * that computes on the grid; the host-only geometry helpers at the end work without one.
 */
#ifndef FTTE_H
#define FTTE_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct ftte_ctx ftte_ctx;

typedef enum {
    FTTE_OK = 0,
    FTTE_ERR_ARG = -1,            /* null pointer, non-positive size, ...                         */
    FTTE_ERR_STATE = -2,          /* call order: grid / opacity not set                           */
    FTTE_ERR_NO_DEVICE = -3,      /* no usable HIP device, or a HIP call failed                    */
    FTTE_ERR_UNSUPPORTED = -4,    /* valid request this build does not implement (see message)     */
    FTTE_ERR_NOT_CUBIC = -5,      /* equiSources.f90:436-439 'base grid needs to be of size n^3'   */
    FTTE_ERR_LEVELS = -6,         /* readCellArray.f90:182 'error in levels'                       */
    FTTE_ERR_PHI = -7,            /* equiSources.f90:1412 'error in phi' (on a quadrant boundary)  */
    FTTE_ERR_THETA = -8,          /* equiSources.f90:1426 'error in theta'                         */
    FTTE_ERR_DOMINANT_AXIS = -9,  /* equiSources.f90:1450 'error in theta or phi' (tie)            */
    FTTE_ERR_PATTERN = -10,       /* transportRoutinesModule.f90:33-36,60-63; equiSources.f90:1523 */
    FTTE_ERR_IZONE = -11,         /* rotateIndices called with izone outside 1..24                 */
    FTTE_ERR_PIXEL = -12,         /* equiSources.f90:2152-2160 'nside/ipix out of range'           */
    FTTE_ERR_RATES = -13,         /* equiSources.f90:3637-3654: a species fraction left [0, 1]     */
    FTTE_ERR_MEMORY = -14,        /* not enough device memory for the request (see message)         */
    FTTE_ERR_STALLED = -15,       /* a one-launch sweep (option "dataflow") stopped making progress; its J is not valid */
    FTTE_ERR_INTERNAL = -16       /* the library caught itself breaking one of its own bounds (see message); outputs untouched */
} ftte_status;

/* ---- lifetime ------------------------------------------------------------------------------ */

/* ndev = 1: one context drives one device (dev_ids[0] = HIP device ordinal; dev_ids may be NULL for the current device).
 *
 * ndev > 1: ONE context, driven by the one host thread the reference is (its direction loop, equiSources.f90:1385-1391, is serial;
 * the directions' only coupling is the sum transportRoutinesModule.f90:953-955), sweeps on dev_ids[0 .. ndev-1].  Such a context
 * takes HOST arrays: ftte_set_grid, ftte_set_opacity, ftte_set_emissivity / ftte_set_source_function, ftte_diffuse_sweep,
 * ftte_diffuse_iteration (plus ftte_set_option, ftte_host_register / _unregister, ftte_counter, ftte_launch_info for the first
 * device's share, ftte_last_error, ftte_destroy); every other entry point returns FTTE_ERR_UNSUPPORTED on it.  The work is split
 * frequency groups first, then directions: with r_nu = gcd(ndev, groups) and r_dir = ndev / r_nu, device k sweeps the groups of
 * frequency slice k mod r_nu for the directions of slice k div r_nu.  A frequency-sharded J_nu is complete where it is computed
 * (8 groups on 8 devices: nothing is exchanged, every device sends its groups home); where directions are split too, the r_dir
 * devices that hold the same groups sum their J by a reduce-scatter over RCCL (librccl.so, loaded on first need) and each sends
 * its piece home.  Where RCCL cannot serve (two entries of dev_ids name the same device -- a test on a one-GPU box --, or no
 * library) the pieces are summed by a kernel that reads the partners' buffers in place; ftte_multi_info says which.
 * J equals the single-device J to the rounding of the sum over directions.  The other way to many GPUs -- one process and one
 * context per GPU, J combined by the host driver (radiativetransfer_amd/distributed.py over torch.distributed) -- stays. */
int ftte_create(ftte_ctx **ctx, int ndev, const int *dev_ids);
/* How the last sweep of a multi-device context combined its devices' J, in words ("" for a single-device context). */
const char *ftte_multi_info(const ftte_ctx *ctx);
int ftte_destroy(ftte_ctx *ctx);
/* Message of the last failing call on this context ("" if none); ctx may be NULL for the
 * message of the last failing ftte_create. */
const char *ftte_last_error(const ftte_ctx *ctx);

/* ---- inputs -------------------------------------------------------------------------------- */

/* The grid: stands in for the tree the reference builds from the cell array
 * (readCellArray.f90:154-187 createFullyThreadedStructure) and for physicalBoxSize
 * (definitionsModule.f90:256).  nx == ny == nz is required, as in the reference.
 * level[ncell]: depth-first leaf list, 0 = base cell.  A list of all zeros (ncell = nx^3) is a
 * uniform grid and takes the tiled sweep kernel; a refined cell array takes the general
 * segment-forest path (setRaysRefined / findNeighbours / transport of the reference).
 * The reference's tree is static over a run: a call with the list the context already holds returns at once and
 * keeps the tree, the sweep plans and the device-resident medium (only box_cm is taken over). */
int ftte_set_grid(ftte_ctx *ctx, int nx, int ny, int nz, int64_t ncell, const int32_t *level, double box_cm);

/* Opacities kappa[nnu][ncell] in cell-array order (host memory), cm^-1.  Stands in for the
 * kappa1..3 fields filled by computeOpacities (equiSources.f90:4977-4980); nnu is free
 * (the reference hard-wires 3 groups, definitionsModule.f90:169-171). */
int ftte_set_opacity(ftte_ctx *ctx, int nnu, const double *kappa);
/* Same, kappa already resident in device memory (not retained beyond the call).  The data must be complete when
 * the call is made (synchronise the stream that produced it); the same holds for the other *_device setters. */
int ftte_set_opacity_device(ftte_ctx *ctx, int nnu, const double *kappa_dev);
/* computeOpacities itself (equiSources.f90:4956-4983) for nnu groups, on the device:
 * kappa_g = HI*beta[0][g] + HeI*beta[1][g] + HeII*beta[2][g] (left to right).
 * HI/HeI/HeII: [ncell] host arrays, beta: [3][nnu] host array (rows: HI = beta24,
 * HeI = beta26, HeII = beta25 of the reference's group tables). */
int ftte_set_species(ftte_ctx *ctx, int nnu, const double *HI, const double *HeI, const double *HeII,
                     const double *beta);
/* Emissivity eta[nnu][ncell] (call after the opacities are set; sized by their nnu: opacities with another nnu switch
 * emission off until it is set again).  NULL selects the reference's
 * hard-wired zero emissivity (transportRoutinesModule.f90:673-675).  Non-NULL switches the sweep to the reference's
 * emission term as written at :676,   Iout = Iin*tmpabs + nemi*tmpemi/dpath   with tmpemi = (1-tmpabs)/kappa
 * (dpath below tau = 1e-10), and to its log-mean (:1044-1048) for the cell intensity.  Replaces any source function. */
int ftte_set_emissivity(ftte_ctx *ctx, const double *eta);
int ftte_set_emissivity_device(ftte_ctx *ctx, const double *eta_dev);
/* Source function S[nnu][ncell]: NOT in the reference (whose emission term is never enabled and is not an emissivity
 * per unit length): Iout = Iin*exp(-tau) + S*(1 - exp(-tau)), the form a source iteration S = (1-eps) J + eps B needs
 * (BASELINE configs[4]).  NULL switches emission off.  Replaces any emissivity. */
int ftte_set_source_function(ftte_ctx *ctx, const double *S);
int ftte_set_source_function_device(ftte_ctx *ctx, const double *S_dev);

/* ---- the sweep ----------------------------------------------------------------------------- */

/* One diffuse-transfer iteration = equiSources.f90:1385-1806 for a caller-supplied direction
 * list: for every direction, fold it (:1395-1454), build the per-layer ray patterns
 * (:1495-1534, setPattern), and sweep all cells (:1572-1796 / transport), accumulating
 * J_nu += w * mean-over-segments(log-mean intensity).
 * phi[ndir] in (0, 2 pi), theta[ndir] in (-pi/2, pi/2) (the reference's un-folded angles, as
 * pix2ang_nest returns them), w[ndir], uvb[nnu] (inflow on every upstream boundary face,
 * definitionsModule.f90:55-56), J[nnu][ncell] host memory, overwritten. */
int ftte_diffuse_sweep(ftte_ctx *ctx, int ndir, const double *phi, const double *theta, const double *w,
                       const double *uvb, double *J);
/* ftte_set_opacity + ftte_diffuse_sweep in one call (the pair the drop-in for the reference's runUVBTransfer block makes on
 * every outer iteration), and faster than the two: on a uniform grid the frequency groups travel in lanes --
 * the first lane is swept while the second one's opacities are still crossing PCIe, and its J goes back while the second is
 * swept.  Same J as the two calls; refined cell arrays and the options that exclude lanes take the two calls internally.
 * kappa[nnu][ncell], J[nnu][ncell] host memory (pageable, or registered with ftte_host_register: DMA in place). */
int ftte_diffuse_iteration(ftte_ctx *ctx, int nnu, const double *kappa, int ndir, const double *phi, const double *theta,
                           const double *w, const double *uvb, double *J);
/* Same with J in device memory.  `stream` is a hipStream_t; NULL = the context's own stream, a blocking stream,
 * i.e. one that is implicitly ordered with the legacy default stream.  The call is asynchronous with respect to the
 * host, ordered on that stream. */
int ftte_diffuse_sweep_device(ftte_ctx *ctx, int ndir, const double *phi, const double *theta, const double *w,
                              const double *uvb, double *J_dev, void *stream);

/* ---- accelerated source iteration -------------------------------------------------------------
 * NOT in the reference (like the source function itself, its emission never being enabled): the build's own definition.
 *
 * The diagonal of the discrete Lambda operator of the sweep with a source function.  A cell's share of a ray segment is
 * S + (Iin - S) g(tau), g = (1 - exp(-tau))/tau; the (up to three) segments of a cell belong to different rays and each takes its
 * Iin from ANOTHER cell or from the inflow, so a cell's own S enters its own J through S (1 - g) alone:
 *     diag[nu][cell] = sum over directions  w/nseg * sum over the cell's segments (1 - g(kappa_nu(cell) * dpath_seg))
 * evaluated with the sweep's own arithmetic in the sweep's own order (segments xy, xz, yz, then the mean, directions in list
 * order): it equals J[cell] of a sweep with S = 1 in that cell and 0 elsewhere and no inflow, bit for bit, on uniform grids and
 * refined cell arrays alike, whatever ftte_set_option says.  0 <= diag < sum of w.  Arguments as ftte_diffuse_sweep takes them
 * (phi, theta, w before folding); diag[nnu][ncell] host memory, cell-array order, overwritten.
 * It goes stale with a new grid, new opacities or another direction list; nothing is cached: recomputing is the caller's
 * decision.  Errors as the sweep's (FTTE_ERR_STATE without grid or opacities); FTTE_ERR_UNSUPPORTED on a multi-device context. */
int ftte_lambda_diagonal(ftte_ctx *ctx, int ndir, const double *phi, const double *theta, const double *w, double *diag);
/* Same with diag in device memory; asynchronous on `stream` (NULL: the context's own), like ftte_diffuse_sweep_device. */
int ftte_lambda_diagonal_device(ftte_ctx *ctx, int ndir, const double *phi, const double *theta, const double *w,
                                double *diag_dev, void *stream);
/* One step of the source iteration S = (1 - eps) J + eps B, element-wise over [nnu][ncell] device arrays, in one pass:
 *     S <- S + ((1 - eps) J + eps B - S) / (1 - (1 - eps) diag)      (in this order of operations, IEEE division)
 * the approximate-operator (Jacobi) update whose fixed point is that of the plain iteration; diag_dev = NULL: the plain update
 * S <- (1 - eps) J + eps B.  B_dev: [nnu] (b_per_cell = 0) or [nnu][ncell].  change[2] (host, may be NULL) receives
 * max |S_new - S_old| and max |S_new|: a measure of progress, not of the error (a slowly converging iteration changes little).
 * A denominator that is not positive (the weights sum to more than 1/(1 - eps)) is FTTE_ERR_ARG naming the first such element;
 * S is then unchanged.  Ordered on `stream`; returns when the step has completed. */
int ftte_source_update_device(ftte_ctx *ctx, int nnu, double epsilon, const double *B_dev, int b_per_cell, const double *J_dev,
                              const double *diag_dev, double *S_dev, double *change, void *stream);

/* ---- point sources ---------------------------------------------------------------------------
 * The `runStellarTransfer` block, equiSources.f90:1256-1370: for each star particle build the rate
 * tables of its population (stellarBetaTable), then send 12 HEALPix rays from the centre of its host
 * cell; a ray splits into its four daughter pixels after rmax(level) cells (startNewLongRay,
 * :3120-3385), crosses cells with drawSegment (:2412-2595) and the neighbour search
 * (find/zoom??Neighbour, :2647-2960), and deposits in every cell it crosses
 * ndot * (R(depth) - R(depth + tau)) for the three photo-reactions, R from the tables
 * (getRatesHydrogenHelium, :4157-4311).
 *
 * Host sequence, mirroring the reference:
 *   ftte_set_grid; ftte_set_medium; ftte_set_zero_rates;
 *   per population: ftte_stellar_beta_table (or ftte_set_rate_tables); ftte_point_sources(stars of it);
 *   ftte_get_point_rates.
 * or, where every star has a population of its own (the reference builds its tables per star from the host cell's
 * metallicity, equiSources.f90:1282-1299), batched:
 *   ftte_set_grid; ftte_set_medium; ftte_set_zero_rates;
 *   ftte_stellar_beta_tables(all populations of the batch) (or ftte_set_population_tables);
 *   ftte_point_sources_populations(stars, the slot each reads); ftte_point_escape;
 *   ftte_get_point_rates.
 * Rates accumulate on the device between ftte_set_zero_rates and ftte_get_point_rates.
 * In front of either, from a star list (equiSources.f90:746-769, :1169-1212, :1282-1293):
 *   ftte_star_catalogue(coordinates, weights); ftte_star_sources -> src_cell, src_ndot, src_abun2;
 *   ftte_star_populations(src_abun2) -> iMetal, coefMetal of each population and the slot each source reads. */

#define FTTE_TABLE_SIZE 14641 /* (ndepth+1)^4 = 11^4, definitionsModule.f90:72-77 */
#define FTTE_MAX_PIXEL_LEVEL 6 /* maxPixelLevel, equiSources.f90:9 */

/* stellarBetaTable(nfbins, frequencyBinWidth, totalIntegral, iSpectrum, coefSpectrum, iMetal, coefMetal),
 * stellarBetaTable.f90:3-289, with the module data it reads passed explicitly, all as the Fortran
 * arrays lie in memory: a_smc(7,5) (read at dustModule.f90:16-21), wavelength(nwave) [cm, ascending],
 * specificLuminosity(nmetal, nspectrum, nwave) (definitionsModule.f90:270; 5 x 37 x 1221 in the
 * reference).  iSpectrum, iMetal are 1-based.  The six tables reactionRate1..3, energyRate1..3 are
 * accumulated on the device over the 399 frequency bins and stay there; total_integral (may be NULL)
 * is the reference's totalIntegral. */
int ftte_stellar_beta_table(ftte_ctx *ctx, const double *a_smc, int nwave, const double *wavelength_cm, int nspectrum,
                            int nmetal, const double *specific_luminosity, int iSpectrum, double coefSpectrum, int iMetal,
                            double coefMetal, double *total_integral);
/* Population slots: npop table sets held side by side, for ftte_point_sources_populations.  The slots are apart from "the
 * current tables" of the calls above, which neither read nor change them.  A slot takes 2 x 6 x FTTE_TABLE_SIZE doubles of device
 * memory (1.4 MB); what does not fit in the free memory is FTTE_ERR_MEMORY, with the byte count in the message, and leaves the
 * slots held as they were.  ftte_counter(ctx, "population_slots") is the number held.
 *
 * ftte_stellar_beta_tables: stellarBetaTable for npop populations (iSpectrum, coefSpectrum, iMetal, coefMetal)[npop] into slots
 * 0..npop-1, replacing any earlier slots.  Per population the host work and the device arithmetic of ftte_stellar_beta_table, so
 * that a slot holds bit for bit what that call stores; frequency grid and cross-sections once, one launch for all tables.
 * total_integral[npop] (may be NULL).  Sets the output cross-sections like ftte_stellar_beta_table. */
int ftte_stellar_beta_tables(ftte_ctx *ctx, const double *a_smc, int nwave, const double *wavelength_cm, int nspectrum,
                             int nmetal, const double *specific_luminosity, int npop, const int *iSpectrum,
                             const double *coefSpectrum, const int *iMetal, const double *coefMetal, double *total_integral);
/* tables[npop][6][FTTE_TABLE_SIZE] computed elsewhere into slots 0..npop-1, replacing any earlier slots (each set laid out as for
 * ftte_set_rate_tables).  The output cross-sections stay what they were (ftte_set_output_sigma). */
int ftte_set_population_tables(ftte_ctx *ctx, int npop, const double *tables);
/* tables[6][FTTE_TABLE_SIZE] of one slot */
int ftte_get_population_tables(ftte_ctx *ctx, int slot, double *tables);
/* Tables computed elsewhere (e.g. by the reference itself): tables[6][FTTE_TABLE_SIZE], order
 * reactionRate1, 2, 3, energyRate1, 2, 3, each the Fortran array (0:ndepth,0:ndepth,0:ndepth,0:ndepth)
 * (tau1, tau2, tau3, tauDust) as it lies in memory. */
int ftte_set_rate_tables(ftte_ctx *ctx, const double *tables);
int ftte_get_rate_tables(ftte_ctx *ctx, double *tables);
/* getRatesHydrogenHelium(reaction, tau1, tau2, tau3, tauDust, numberRate, heatingRate),
 * equiSources.f90:4157-4311, for nsample depth tuples and all three reactions, evaluated on the device:
 * tau[nsample][4], rates[nsample][3][2] = (numberRate, heatingRate) per reaction.
 * dust_approximation: 0 noDust, 1 dust ~ HI, 2 dust ~ total hydrogen (definitionsModule.f90:87). */
int ftte_get_rates_hydrogen_helium(ftte_ctx *ctx, int dust_approximation, int nsample, const double *tau, double *rates);
/* Cell fields the tracer reads (zoneType HI, HeI, HeII, rho, abun2, definitionsModule.f90:163-168), cell-array
 * order, ncell each.  rho / abun2 may be NULL when the dust approximation does not read them. */
int ftte_set_medium(ftte_ctx *ctx, const double *HI, const double *HeI, const double *HeII, const double *rho,
                    const double *abun2, int dust_approximation);
int ftte_set_medium_device(ftte_ctx *ctx, const double *HI, const double *HeI, const double *HeII, const double *rho,
                           const double *abun2, int dust_approximation);
/* setZeroRates, equiSources.f90:4128-4155 */
int ftte_set_zero_rates(ftte_ctx *ctx);
/* localizeCellFromStar, equiSources.f90:2597-2620: the star's call sequence position(1:3*(level+1)) (base
 * indices 1..n, then child indices 1..2 per level) -> 0-based cell-array index of its host cell. */
int ftte_locate_cell(ftte_ctx *ctx, int level, const int32_t *position, int64_t *cell);
/* The star catalogue on the device.  Stars are merged by HOST LEAF.  The reference merges by a key that two leaves of different
 * depth can share (base cell 10 b + d, unrefined, and child d of base cell b), and then lets an unstable sort choose the survivor:
 * that is not reproduced.
 *
 * :746-769 and :1169-1212 for nstars stars. xyz[nstars][3] in the units of lo/hi (the reference's xa..zb);
 * weight[nstars] >= 0 or NULL (= 1 each: the age filter :773-783 stays with the caller).
 * star_cell[nstars] (may be NULL): host leaf, -1 outside the box.
 * *nsrc: leaves holding weight > 0; *outside: stars outside.
 * Results stay on the device for ftte_star_sources.
 * A star is inside where 0 <= int(x * n) < n along every axis of the unit cube, int() truncating as the reference's: -0.0 and
 * nextafter(1, 0) are inside, 1.0, NaN and +-inf outside.  FTTE_ERR_ARG: hi <= lo or either not finite, a negative weight,
 * weights beyond 2^31 - 1 in sum, nstars > 2^31 - 1 (ftte_last_error names the first offender); the last catalogue stays. */
int ftte_star_catalogue(ftte_ctx *ctx, int64_t nstars, const double *xyz, const double lo[3], const double hi[3],
                        const int32_t *weight, int64_t *star_cell, int64_t *nsrc, int64_t *outside);
/* The sources of the LAST ftte_star_catalogue, ascending src_cell; any pointer may be NULL.
 * src_ndot = (double)(float)weight (:1306); src_first_star = lowest star index with weight > 0 in the leaf;
 * src_abun2 needs a medium with abun2 (else FTTE_ERR_STATE). */
int ftte_star_sources(ftte_ctx *ctx, int64_t nsrc, int64_t *src_cell, int32_t *src_weight, double *src_ndot,
                      int64_t *src_first_star, double *src_abun2);
/* host only, no context: :1282-1293 per source, then one slot per distinct (iMetal, coefMetal) bit pattern in order
 * of first appearance: src_slot[nsrc], *npop, pop_first[npop] = a source that carries slot p's parameters (room for nsrc entries
 * always suffices).  metallicity[nmetal] ascending, nmetal >= 2; iMetal is 1-based and at most nmetal - 1.  Outputs may be NULL. */
int ftte_star_populations(int nmetal, const double *metallicity, int64_t nsrc, const double *abun2,
                          int32_t *iMetal, double *coefMetal, int32_t *src_slot, int64_t *npop, int64_t *pop_first);
/* host only: inverse of ftte_locate_cell -- leaf -> level and call sequence position(1:3*(level+1)); position (may be NULL)
 * needs room for the leaf's level, 183 entries always suffice */
int ftte_cell_position(ftte_ctx *ctx, int64_t cell, int *level, int32_t *position);
/* The per-star loop body, equiSources.f90:1268-1329, for nsrc stars that share the current tables:
 * src_cell[nsrc] host cells (0-based cell-array index), src_ndot[nsrc] = float(weight).  Adds into the device
 * rates.  highest_pixel_level (may be NULL): the largest value of the reference's highestPixelLevel over
 * these stars.  Deposition uses fp64 atomics: the last bits of the sums depend on the run. */
int ftte_point_sources(ftte_ctx *ctx, int nsrc, const int64_t *src_cell, const double *src_ndot, int *highest_pixel_level);
/* ftte_point_sources with star s reading the tables of population slot src_slot[s] (0-based) instead of the current tables.  Adds
 * into the same rates and feeds ftte_point_escape and ftte_point_ray_steps the same way.  highest_pixel_level[nsrc] (may be NULL)
 * is per star: the reference resets highestPixelLevel for every star (equiSources.f90:1266) and prints it in its `src:` line.
 * A slot outside those held is FTTE_ERR_ARG (the message names the first such star), no slots FTTE_ERR_STATE; otherwise the
 * preconditions of ftte_point_sources.  On an error the rates are unchanged. */
int ftte_point_sources_populations(ftte_ctx *ctx, int nsrc, const int64_t *src_cell, const double *src_ndot, const int32_t *src_slot,
                                   int *highest_pixel_level);
/* The escape bookkeeping startNewLongRay keeps per star (equiSources.f90:3198-3233, :3336-3345; reset per star at :1267-1270), for
 * the nsrc stars of the LAST ftte_point_sources / ftte_point_sources_populations call, in its order: remaining[nsrc][7] = ndotRemaining and boundary[nsrc][7] =
 * ndotBoundary at outputRadius = 0.1, 0.3, 1, 3, 10, 30, 100 kpc (equiSources.f90:10), dust[nsrc] = ndotDust, spectrum[nsrc][300] =
 * ndotSpectrum at the last radius (zero unless the output cross-sections are known: ftte_stellar_beta_table computes them,
 * ftte_set_output_sigma hands them over), fraction[nsrc][7] as the main program forms it for its `src:` line (:1342-1348:
 * remaining / (ndot - boundary), or 0 once a whole photon unit has left through the box).  Any pointer may be NULL.  The sums are
 * accumulated with fp64 atomics like the rates. */
int ftte_point_escape(ftte_ctx *ctx, int nsrc, double *remaining, double *boundary, double *dust, double *spectrum, double *fraction);
/* outputSigma24, outputSigma25, outputSigma26, outputSigmaDust (definitionsModule.f90:293-294; stellarBetaTable.f90:119-152),
 * sigma[4][300] in that order, for tables that came in through ftte_set_rate_tables */
int ftte_set_output_sigma(ftte_ctx *ctx, const double *sigma);
/* rates[6][ncell]: krate24, krate25, krate26, crate24, crate25, crate26 (zoneType, definitionsModule.f90:166) */
int ftte_get_point_rates(ftte_ctx *ctx, double *rates);
/* The same [6][ncell] in device memory: a copy in the interface's layout (the tracer accumulates into a packed array),
 * valid until the rates change */
int ftte_point_rates_device(ftte_ctx *ctx, double **rates_dev);
/* Replace the device-resident rates, e.g. by the sum over the GPUs that traced different stars; same layout */
int ftte_set_point_rates(ftte_ctx *ctx, const double *rates);
/* cell crossings (ray segments drawn) of the last ftte_point_sources, all rays of all stars */
long long ftte_point_ray_steps(const ftte_ctx *ctx);
/* rmax(1:30), equiSources.f90:296-309 (formula, halved) */
int ftte_rmax(double *rmax30);
/* uvbBetaTable(nfreq, freqdel, alpha), uvbBetaTable.f90:3-305 (host): the three frequency groups [nu1, nu2], [nu2, nu3],
 * [nu3, inf) with power-law slopes alpha[3].  beta[3][3] = [species HI, HeI, HeII][group] (group%beta24, beta26, beta25:
 * the matrix ftte_set_species / ftte_compute_opacities take; computeOpacities uses its lower triangle,
 * equiSources.f90:4977-4980), ksi[3][3] = [group][ksi24, ksi25, ksi26] (what ftte_solve_rate_equations takes),
 * gamma[3][3] = [group][gammaHI, gammaHeI, gammaHeII].  The reference calls it with nfbins = 400, frequencyBinWidth = 0.02
 * (equiSources.f90:253). */
int ftte_uvb_beta_table(int nfreq, double freqdel, const double *alpha, double *beta, double *ksi, double *gamma);
/* coll_rates(T, k1, ..., k19, recombinationType), coll_rates.f:42-150 (host): the six rate coefficients the equilibrium uses,
 * k[6] = k1..k6 [cm^3/s]; recombination_type 1 = case A, 2 = case B (the reference's setting, definitionsModule.f90:48) */
int ftte_coll_rates(double T, int recombination_type, double *k);
/* k1a..k6a(nratec) as calc_rates.f:324-337 fills them, k[6][nratec], and logtem0, logtem9, dlogtem of equiSources.f90:174-176:
 * what ftte_set_rate_coefficients takes (the reference: nratec = 5000, temstart = 1., temend = 1.e8) */
int ftte_rate_coefficient_tables(int nratec, double temstart, double temend, int recombination_type, double *k, double *logtem0,
                                 double *logtem9, double *dlogtem);
/* The thirteen cooling coefficients as calc_rates.f:414-544 fills them with the flags as compiled (:155), and compa (:619), on the
 * temperature grid of ftte_rate_coefficient_tables (host, no context): c[13][nratec] in the order of equiSources.f90:3975-3987 --
 * ceHI, ceHeI, ceHeII, ciHI, ciHeI, ciHeIS, ciHeII, reHII, reHeII1, reHeII2, reHeIII, brem, lineHI -- what
 * ftte_set_cooling_coefficients takes.  Case B (recombination_type 2) interpolates the reference's two data files, which the
 * caller hands over as the files hold them: mellema[81][2] = columns 1 and 3 of HII-ktbetas.tab, gnedin[201][3] = columns 1, 3, 5
 * of cratesHe.res; FTTE_ERR_ARG without them.  Case A needs neither (NULL). */
int ftte_cooling_coefficient_tables(int nratec, double temstart, double temend, int recombination_type, const double *mellema,
                                    const double *gnedin, double *c, double *compa);
/* uniformTable(nfreq, freqdel, alphaQuasar, alphaStellar), uniformTable.f90:1-200 (host): the two power-law components of the
 * uniform background.  ksi[2][3] = [quasar, stellar][ksi24, ksi25, ksi26], gamma[2][3] = [quasar, stellar][gammaHI, gammaHeI,
 * gammaHeII]; uniformQuasar*ksi[0][x] + uniformStellar*ksi[1][x] is the `uniform` argument of ftte_solve_rate_equations. */
int ftte_uniform_table(int nfreq, double freqdel, double alpha_quasar, double alpha_stellar, double *ksi, double *gamma);
/* dustCrossSection(lambda [micron]), dustModule.f90:30-73, SMC curve; a_smc(7,5) Fortran order */
double ftte_dust_cross_section(double lambda_micron, const double *a_smc);

/* ---- ionisation equilibrium --------------------------------------------------------------------
 * solveRateEquations(currentCell, nx, runUVBTransfer), equiSources.f90:3459-3677, for every leaf: the
 * consumer of J (Jmean1..3) and of the point-source rates (krate24..26), and the producer of the next
 * iteration's HI, HeI, HeII (driver loop equiSources.f90:1811-1819).  Per cell: photo-rates per
 * absorber, collisional rate coefficients interpolated in log T, bisection on the electron density.
 * The update works on the device-resident medium of ftte_set_medium (which must have been given rho)
 * and leaves the new HI, HeI, HeII there; every operation is the reference's, in its order. */

/* k1a..k6a(nratec) of calc_rates / coll_rates (calc_rates.f:324-337) and the table's logtem0, logtem9,
 * dlogtem (equiSources.f90:174-176) */
int ftte_set_rate_coefficients(ftte_ctx *ctx, int nratec, double logtem0, double logtem9, double dlogtem, const double *k1a,
                               const double *k2a, const double *k3a, const double *k4a, const double *k5a, const double *k6a);
/* zoneType%tgas per leaf [K]: its logarithm, taken on the host, for the chemistry, and the temperature itself for the thermal balance */
int ftte_set_temperature(ftte_ctx *ctx, const double *tgas);
/* run_uvb_transfer != 0 (:3545-3553): J[3][ncell] (Jmean1..3) and ksi[3][3] = (ksi24, ksi25, ksi26) of group1..3
 * (normCrossSectionType, definitionsModule.f90:94-103); uniform may be NULL.
 * run_uvb_transfer == 0 (:3554-3562): uniform[3] = uniformQuasar*quasar%ksi2x + uniformStellar*stellar%ksi2x for
 * x = 4, 5, 6, applied where the Lyman-limit mean free path is at least self_shielding_threshold; J, ksi may be NULL.
 * use_point_rates != 0: krate24..26 of the device-resident point-source rates enter (:3520-3542); 0: they are zero.
 * max_change (may be NULL): largest change of HI/nH, HeI/nHe, HeII/nHe over the cells.
 * FTTE_ERR_RATES where the reference prints the species and stops; the medium is then left unchanged. */
int ftte_solve_rate_equations(ftte_ctx *ctx, int run_uvb_transfer, const double *J, const double *ksi, const double *uniform,
                              double self_shielding_threshold, int use_point_rates, double *max_change);
/* Same with J in device memory, e.g. the output of ftte_diffuse_sweep_device: the iteration stays on the device */
int ftte_solve_rate_equations_device(ftte_ctx *ctx, int run_uvb_transfer, const double *J_dev, const double *ksi,
                                     const double *uniform, double self_shielding_threshold, int use_point_rates,
                                     double *max_change);
/* Time-dependent ionisation at fixed temperature: HI, HeI, HeII of every leaf advanced over dt_s seconds instead of replaced by
 * their equilibrium.  Arguments, preconditions and error texts those of ftte_solve_rate_equations.  Per cell: the incoming state
 * clipped to the elements' budgets (HI <= nH, HeI <= nHe, HeII <= nHe - HeI, none negative); the rates per absorber formed from
 * it exactly as the equilibrium update forms them, and held fixed for the whole call; `substeps` backward-Euler steps of
 * dt_s / substeps, each closed by a bisection on the electron density run until its midpoint is an end of the bracket.  First
 * order in the step; its stationary state is the equilibrium of the same rates (dt_s = 1e40 gives it to rounding).  The coupling
 * to the transfer is explicit: J and the point-source rates are the caller's, from the state before the call.
 * FTTE_ERR_ARG unless dt_s is finite and > 0 and 1 <= substeps <= 4096.  FTTE_ERR_RATES, the first failing cell named and the
 * medium unchanged, where a species comes out not finite or outside its element's budget by more than rounding (an empty
 * cell) or a bisection does not settle in 4096 steps.  max_change as there; ftte_rate_equation_steps counts the bisection
 * steps of all substeps. */
int ftte_advance_rate_equations(ftte_ctx *ctx, double dt_s, int substeps, int run_uvb_transfer, const double *J, const double *ksi,
                                const double *uniform, double self_shielding_threshold, int use_point_rates, double *max_change);
/* Same with J in device memory: a time step stays on the device */
int ftte_advance_rate_equations_device(ftte_ctx *ctx, double dt_s, int substeps, int run_uvb_transfer, const double *J_dev,
                                       const double *ksi, const double *uniform, double self_shielding_threshold,
                                       int use_point_rates, double *max_change);
/* ---- thermal balance: thermalEquilibrium (equiSources.f90:3870-4042) and the temperature over a time step -----------------
 * Per cell one statement shared by host and device (csrc/ftte_thermal_math.h).  The reference's: the locals HI .. de (:3907-3925),
 * the heating of the uniform background behind the self-shielding test (:3929-3940), the interpolation of the thirteen cooling
 * coefficients (:3946-3987), edot (:3991-4029, without the two terms it multiplies by literal zeros) and hydroHeating
 * (:4030-4038); its write-back of the clipped helium into the cell (:3914-3918) is not made: no thermal call changes a species.
 * The build's own: the heating by the transfer's J and by the point sources, formed as solveRateEquations forms the ionisation
 * rates, and the temperature step.  The rate arguments are those of ftte_solve_rate_equations with the heating integrals in place
 * of ksi: gamma[3][3] = [group][gammaHI, gammaHeI, gammaHeII] of ftte_uvb_beta_table (crate24 += t1 g[0][0] + t2 g[1][0] +
 * t3 g[2][0], crate26 += t2 g[1][1] + t3 g[2][1], crate25 += t3 g[2][2], t = 4 pi J), uniform_gamma[3] = uniformQuasar*quasar%gamma +
 * uniformStellar*stellar%gamma of HI, HeII, HeI (ftte_uniform_table), use_point_rates: crate24..26 of the device-resident rates.
 * Preconditions those of ftte_solve_rate_equations plus ftte_set_cooling_coefficients. */

/* The temperature per leaf [K] as it stands on the device: what ftte_set_temperature gave, or the last ftte_advance_temperature's */
int ftte_get_temperature(ftte_ctx *ctx, double *tgas);
/* c[13][nratec] of ftte_cooling_coefficient_tables, compa, and currentRedshift: comp1 = compa (1+z)^4, comp2 = 2.73 (1+z).
 * FTTE_ERR_STATE before ftte_set_rate_coefficients, FTTE_ERR_ARG unless nratec is that call's: the two share one temperature grid
 * (another nratec there drops these coefficients). */
int ftte_set_cooling_coefficients(ftte_ctx *ctx, int nratec, const double *c, double compa, double redshift);
/* thermalEquilibrium for every leaf, at ftte_log of its temperature: heating = crate (:3940), cooling = minus the cooling sum,
 * hydro_heating = max(cooling - heating, 0) [erg/(s cm^3)], ncell each, each may be NULL; hydroHeating stays on the device.  With
 * run_uvb_transfer == 0 and use_point_rates == 0 it is the reference's start-up pass (:1025-1033).  FTTE_ERR_RATES (first
 * failing cell named, nothing stored) where a temperature is not positive and finite or a result is not finite. */
int ftte_thermal_equilibrium(ftte_ctx *ctx, int run_uvb_transfer, const double *J, const double *gamma, const double *uniform_gamma,
                             double self_shielding_threshold, int use_point_rates, double *heating, double *cooling,
                             double *hydro_heating);
int ftte_thermal_equilibrium_device(ftte_ctx *ctx, int run_uvb_transfer, const double *J_dev, const double *gamma,
                                    const double *uniform_gamma, double self_shielding_threshold, int use_point_rates, double *heating,
                                    double *cooling, double *hydro_heating);
/* The temperature of every leaf advanced over dt_s seconds, isochoric, the species held fixed (the chemistry is advanced by its
 * own calls: operator-split, explicit).  Heat capacity per volume c = kB (nH + nHe + de)/(gamma - 1); the rates per absorber are
 * formed once per call; use_hydro_heating != 0 adds the leaf's stored hydroHeating to the net rate.  The incoming T is clipped to
 * [tmin, tmax]; each of `substeps` backward-Euler steps of h = dt_s/substeps solves F(T) = (T - T0) - (h/c) (edot(T) + hydro) = 0:
 * F(T0) == 0 leaves T0; net heating brackets [T0, tmax] (T1 = tmax if F(tmax) <= 0), net cooling [tmin, T0] (T1 = tmin if
 * F(tmin) > 0); else bisection in T until the midpoint is an end of the bracket, so that F(T1) <= 0 < F(nextafter(T1)).  The
 * cooling curve is not monotonic: of several roots the step returns the one its bracket, on the gas's own side of T0, closes on.
 * Afterwards the leaf's temperature and its logarithm (ftte_log) are the device's: the next chemistry call reads them.
 * max_change (may be NULL): largest |T1 - T0|/T0, T0 the clipped incoming temperature; ftte_rate_equation_steps counts the bisection
 * steps.  FTTE_ERR_ARG unless dt_s is finite and > 0, 1 <= substeps <= 4096 and 0 < tmin < tmax are finite; FTTE_ERR_STATE when
 * use_hydro_heating is set and no ftte_thermal_equilibrium has run on this grid; FTTE_ERR_RATES, the first failing cell named and
 * nothing changed, where a temperature, a heat capacity or an F is not finite or a bisection does not settle in 4096 steps. */
int ftte_advance_temperature(ftte_ctx *ctx, double dt_s, int substeps, double tmin, double tmax, int use_hydro_heating,
                             int run_uvb_transfer, const double *J, const double *gamma, const double *uniform_gamma,
                             double self_shielding_threshold, int use_point_rates, double *max_change);
int ftte_advance_temperature_device(ftte_ctx *ctx, double dt_s, int substeps, double tmin, double tmax, int use_hydro_heating,
                                    int run_uvb_transfer, const double *J_dev, const double *gamma, const double *uniform_gamma,
                                    double self_shielding_threshold, int use_point_rates, double *max_change);
/* Species and temperature of every leaf advanced TOGETHER over dt_s seconds (csrc/ftte_thermochem_math.h; the build's own -- the
 * reference has no time step, and its commented-out coupled solver is not restated).  Where the pair ftte_advance_rate_equations,
 * ftte_advance_temperature runs the chemistry of the whole step at the temperature of its start and the thermal step at the
 * species of its end, this call takes the two implicit steps in turn over subcycles that each leaf chooses for itself.  Per leaf,
 * once: the state clipped to the elements' budgets, the ionisation rates per absorber as ftte_advance_rate_equations forms
 * them, the heating rates per absorber as ftte_advance_temperature forms them from the incoming state, T clipped to [tmin,
 * tmax]; all six rates stay fixed for the call (the radiation is explicit: J and the point rates are the caller's).  Subcycle s,
 * while time remains: the coefficients at the stored logarithm (s = 0) or at ftte_log(T); the time scale tau = min over HI, HeI,
 * HeII of max(species, 0.2 element)/|d species/dt| and T/|dT/dt|; h = min(remaining, max(eta tau, remaining/(max_subcycles - s)))
 * -- eta = 0 is max_subcycles equal subcycles, and no leaf takes more than max_subcycles; the chemistry's step over h, then the
 * temperature's over h with the new species.  First order in h.  With max_subcycles = 1 the species are those of
 * ftte_advance_rate_equations(dt_s, 1) bit for bit, and T that of ftte_advance_temperature(dt_s, 1) after it where the heating per
 * absorber does not depend on the state (J without point rates).
 * Arguments: those of the two calls -- ksi and uniform as ftte_solve_rate_equations takes them, gamma and uniform_gamma as
 * ftte_thermal_equilibrium does; preconditions those of both.  max_change (may be NULL): [0] the largest change of a species
 * fraction, [1] the largest |T1 - T0|/T0.  subcycles (may be NULL): [0] the sum over the leaves, [1] the largest count of a leaf,
 * [2] the leaves in which the even split of the remaining time (the cap) decided a subcycle.  ftte_rate_equation_steps counts the
 * bisection steps of both kinds.  Afterwards the species are the medium's and T and its logarithm the device's.
 * FTTE_ERR_ARG unless dt_s is finite and > 0, eta finite and >= 0, 1 <= max_subcycles <= 4096 and 0 < tmin < tmax finite;
 * FTTE_ERR_STATE as ftte_advance_temperature; FTTE_ERR_RATES, the first failing leaf named and medium, temperature and logarithm
 * untouched, where either step fails in any subcycle. */
int ftte_advance_thermochemistry(ftte_ctx *ctx, double dt_s, double eta, int max_subcycles, double tmin, double tmax,
                                 int use_hydro_heating, int run_uvb_transfer, const double *J, const double *ksi, const double *gamma,
                                 const double *uniform, const double *uniform_gamma, double self_shielding_threshold, int use_point_rates,
                                 double *max_change, int64_t *subcycles);
int ftte_advance_thermochemistry_device(ftte_ctx *ctx, double dt_s, double eta, int max_subcycles, double tmin, double tmax,
                                        int use_hydro_heating, int run_uvb_transfer, const double *J_dev, const double *ksi,
                                        const double *gamma, const double *uniform, const double *uniform_gamma,
                                        double self_shielding_threshold, int use_point_rates, double *max_change, int64_t *subcycles);
/* per_leaf[ncell]: the subcycles each leaf took in the last ftte_advance_thermochemistry* that got through on this grid;
 * FTTE_ERR_STATE before any */
int ftte_get_subcycles(ftte_ctx *ctx, int32_t *per_leaf);

/* ---- diffuse recombination radiation: a source function from the gas state (csrc/ftte_recombination_math.h) -----------------
 *
 * The build's own (the reference's emissivity is hard-wired to zero, transportRoutinesModule.f90:673-675): recombinations to
 * the ground states of HI, HeI, HeII emit ionising photons, and one pass over the leaves turns the device-resident gas state into
 * the source function the sweep carries.  Per leaf, with the species clipped to the elements' budgets as ftte_advance_rate_equations
 * clips them, HII = nh - HI, HeIII = nhe - HeI - HeII, de = HII + HeII + 2 HeIII and g[0..2] interpolated at the leaf's stored
 * logarithm of the temperature as the rate coefficients are:
 *   R = g de (HII, HeII, HeIII)                                        recombinations to ground per volume and second
 *   E[j] = share[0][j] R[0] + share[1][j] R[1] + share[2][j] R[2]      photons emitted into group j
 *   D[0] = HI ksi[0][0],  D[1] = HI ksi[1][0] + HeI ksi[1][2],  D[2] = HI ksi[2][0] + HeII ksi[2][1] + HeI ksi[2][2]
 *   S[j] = E[j] / (4 pi D[j]),  0 where D[j] == 0
 * D is the leaf's photon capture per unit 4 pi J as ftte_solve_rate_equations evaluates it, so a leaf bathed in J = S re-absorbs
 * exactly E[j]: photon number is conserved against the chemistry, whatever the mix of absorbers.  A (leaf, group) with E > 0 and
 * D == 0 is "lost": nothing there absorbs the group, so the sweep's S (1 - exp(-tau)) cannot emit it. */

/* g[3][nratec]: the coefficients of recombination to the ground states of HI, HeI, HeII [cm^3/s] on the temperature grid of
 * ftte_set_rate_coefficients.  FTTE_ERR_STATE before that call; FTTE_ERR_ARG unless nratec is that call's, or if an entry is
 * negative or not finite.  Another nratec there drops this table, as it drops the cooling coefficients. */
int ftte_set_ground_recombination(ftte_ctx *ctx, int nratec, const double *g);
/* The source function of every leaf, written straight into the context's emission field in cell-array order; on success the next
 * sweep runs with it, on uniform grids, refined grids and with every option, exactly as after ftte_set_source_function_device with
 * the same values.  ksi[3][3] = [group][ksi24, ksi25, ksi26] of ftte_uvb_beta_table; share[3][3] = [ion][group], every entry in
 * [0, 1] and every row sum <= 1 (else FTTE_ERR_ARG).  S[3][ncell] (host; S_dev: device) receives a copy and may be NULL; *lost
 * the count of lost (leaf, group) pairs, may be NULL.
 * FTTE_ERR_STATE, the text naming the missing call, before ftte_set_grid, ftte_set_medium with rho, ftte_set_temperature,
 * ftte_set_rate_coefficients, ftte_set_ground_recombination, or opacities with nnu == 3 (they size the emission field).
 * FTTE_ERR_RATES, the first such leaf named, where a density is not positive and finite or an electron density or an S is not
 * finite; the emission state is then what it was.  How: while no emission is in force the pass writes the field's own buffer,
 * which nothing reads, and emission is switched on only once no leaf has failed (a time loop that switches emission off after each
 * step's sweep, ftte_set_source_function(ctx, NULL), always takes this way); while one is in force the pass writes a buffer of its
 * own, which is copied into the field only once no leaf has failed. */
int ftte_recombination_source(ftte_ctx *ctx, const double *ksi, const double *share, double *S, int64_t *lost);
int ftte_recombination_source_device(ftte_ctx *ctx, const double *ksi, const double *share, double *S_dev, int64_t *lost);
/* HI, HeI, HeII of the device-resident medium, ncell each */
int ftte_get_medium(ftte_ctx *ctx, double *HI, double *HeI, double *HeII);
/* computeOpacities (equiSources.f90:4956-4983) on the device-resident medium: kappa[g] = HI beta[0][g] + HeI beta[1][g] +
 * HeII beta[2][g]; equivalent to ftte_set_species with the medium's arrays, without the host round trip */
int ftte_compute_opacities(ftte_ctx *ctx, int nnu, const double *beta);
/* assignUvbRadiation(currentCell), transportRoutinesModule.f90:1056-1093: the optically thin alternative to the sweep (not called
 * in the reference's loop): J[g][cell] = uvb[g] where the Lyman-limit mean free path 1/(min(HI, psi rho/mh) 6.3e-18 + HeI 7.42e-18 +
 * HeII 1.58e-18) of the device-resident medium is at least the threshold, else 0.  J[nnu][ncell]. */
int ftte_assign_uvb_radiation(ftte_ctx *ctx, int nnu, const double *uvb, double self_shielding_threshold, double *J);
int ftte_assign_uvb_radiation_device(ftte_ctx *ctx, int nnu, const double *uvb, double self_shielding_threshold, double *J_dev);
/* bisection steps of the last ftte_solve_rate_equations*, ftte_advance_rate_equations*, ftte_advance_temperature*, ftte_advance_thermochemistry* or ftte_initial_ionization_equilibrium, summed over the cells (and
 * over the passes of the latter) */
long long ftte_rate_equation_steps(const ftte_ctx *ctx);
/* The start-up ionisation equilibrium, equiSources.f90:1008-1022: initialIonizationEquilibrium (:3679-3868) `passes` times
 * for every leaf (the reference: 2), each pass starting from the last one's HI, HeI, HeII, on the device-resident medium.
 * Preconditions those of ftte_solve_rate_equations (rate coefficients, temperature, a medium with rho).  The rates are the
 * uniform background's alone, uniform[3] as there, where the Lyman-limit mean free path is at least self_shielding_threshold
 * (:3731-3743); unlike solveRateEquations the bracket starts at 1.e-20, its lower residual is never updated, and the
 * bisection runs until HeI stops changing.  neutral_fraction (may be NULL): neutralHydrogenMass / totalHydrogenMass of
 * computeMass over the result, what :1022 prints.  FTTE_ERR_RATES (first failing cell named, medium unchanged) where the
 * reference stops (:3809-3818, :3832-3843) or where the bisection does not settle in 4096 steps. */
int ftte_initial_ionization_equilibrium(ftte_ctx *ctx, const double *uniform, double self_shielding_threshold, int passes,
                                        double *neutral_fraction);
/* computeMass (equiSources.f90:4369-4393) over the device-resident medium: neutralHydrogenMass = sum HI mh cs^3 / msun and
 * totalHydrogenMass = sum psi rho cs^3 / msun [msun], cs the leaf's size; the ratio is the loop's `time` line (:1820-1834).
 * Every term is the reference's; the sums are deterministic (a fixed order, not the reference's sequential one). */
int ftte_hydrogen_mass(ftte_ctx *ctx, double *neutral_msun, double *total_msun);

/* ---- start-up expansion of HII regions ---------------------------------------------------------------
 * equiSources.f90:1035-1069, behind `expansionFlag` (definitionsModule.f90:86: .false. in the shipped source, a compile-time
 * switch; the code behind it is complete and called from the driver).  For every star with weight > 0 the reference lowers
 * rhoCoef in every leaf inside the star's final HII radius that is not denser than 1.0001 times the star's host leaf
 * (findExpansion, :4431-4474), then scales rho, HI, HeI, HeII by rhoCoef where it is below 1 (applyExpansion, :4476-4503). */

/* computeExpansionParameters(nh), equiSources.f90:4395-4429 (host, no context) */
int ftte_expansion_parameters(double nh, double *final_radius_cm, double *density_coefficient);

/* equiSources.f90:1035-1069 on the device-resident medium of ftte_set_medium (needs rho).
 * src_cell[nsrc]: host leaves of the stars with weight > 0 (what ftte_locate_cell returns; duplicates allowed).
 * params: NULL, or [nsrc][3] = finalRadius [cm], densityCoefficient, sourceTotalHydrogenDensity per star, used as given.
 * rho_coef (may be NULL): [ncell], the reference's rhoCoef.  nchanged (may be NULL): leaves with rhoCoef < 1.
 * With params == NULL the host leaves' rho is fetched from the device and the parameters are computed on the host (libm) from
 * nh = psi rho / mh; a host leaf whose density is not positive and finite is FTTE_ERR_ARG naming the source, as are nsrc < 0 and a
 * src_cell outside [0, ncell).  FTTE_ERR_STATE without a grid or a medium with rho.  On any error the medium is unchanged.
 * nsrc == 0 succeeds: nothing changes, rho_coef is all ones.  tgas and abun2 are not touched.  The opacities are the caller's
 * (ftte_compute_opacities), as after ftte_solve_rate_equations.  The result is the same bits run after run: rhoCoef is a minimum
 * over the stars.  ftte_counter(ctx, "expansion_exact_tests"): star-leaf pairs the last call put through the exact test (the
 * rest were ruled out a workgroup of leaves at a time). */
int ftte_expand_hii_regions(ftte_ctx *ctx, int nsrc, const int64_t *src_cell, const double *params,
                            double *rho_coef, int64_t *nchanged);
/* rho of the device-resident medium, ncell */
int ftte_get_density(ftte_ctx *ctx, double *rho);

/* ---- grid ingest (no device needed) -----------------------------------------------------------------
 * What the reference does between reading its grid file and the first transfer (equiSources.f90:427-618,
 * placeCellProjectWithVelocity :1870-1974): per refinement level a list of SPH-projected cells -- position [kpc], log10 of
 * temperature, hydrogen density and neutral fraction, optionally velocities and four abundances -- becomes the octree, and the
 * octree the cell array in writeCell's order (:4044-4079), the order ftte_set_grid, ftte_set_medium and the .dat file take.
 * Level 1 must fill an n^3 base grid (FTTE_ERR_NOT_CUBIC otherwise, :436-439); a cell of level L lies L-1 refinements deep;
 * cells of a refined cell that no list covers keep their parent's state, as in the reference.  The HDF4 container the
 * reference reads the lists from (:316-423) is not read here: the lists are handed over as arrays. */
typedef struct {
    int64_t ncell;
    const float *pos;            /* (ncell,3) as the Fortran array lies: all x, then all y, then all z [kpc] */
    const float *lT, *lnH, *lx;  /* log10 T [K], log10 n_H [cm^-3], log10 neutral fraction */
    const float *vel;            /* (ncell,3) or NULL (the reference's readKinematics) */
    const float *abun;           /* (ncell,4) or NULL (readMetals); column 2 becomes abun2, smoothed on level 1 (:526-578) */
} ftte_level_list;
typedef struct ftte_cellarray ftte_cellarray;
int ftte_ingest_levels(int nlevels, const ftte_level_list *lists, ftte_cellarray **out);
/* base grid size, number of leaves, physicalBoxSize [cm] (:481) */
int ftte_cellarray_info(const ftte_cellarray *a, int *nx, int64_t *ncell, double *box_cm, int *has_velocity, int *has_metals);
/* the leaf arrays, cell-array order, as the tree holds them (binary64); any pointer may be NULL.  tgas and rho are zoneType's
 * fields; abun2 is 0.02 everywhere without metals (:1958). */
int ftte_cellarray_fields(const ftte_cellarray *a, int32_t *level, double *HI, double *HeI, double *HeII, double *tgas, double *rho,
                          double *velx, double *vely, double *velz, double *abun2);
void ftte_cellarray_free(ftte_cellarray *a);

/* ---- analysis: how the reference looks at a result, on the device-resident medium ------------------
 * Each call reads the medium's fields and the tree where they are (no copy is kept, so a map made after ftte_set_medium, an
 * equilibrium update or ftte_expand_hii_regions shows the new medium) and needs a single-device context; a multi-device context
 * never holds a medium (ftte_set_medium is refused on it), so all of them return FTTE_ERR_UNSUPPORTED there.
 * What they keep on the device belongs to the context, is released by ftte_set_grid with another grid and counts in
 * ftte_counter("device_objects").  Refusals: FTTE_ERR_IZONE for izone outside 1..24; FTTE_ERR_ARG for non-positive map sizes,
 * zoom <= 0, zslice outside [0, 1) or a window whose pixels leave the box (the reference indexes out of bounds there);
 * FTTE_ERR_STATE without a medium (ftte_set_medium), for the projection and the censuses without its density.
 *
 * Maps.  map[i + nxmap*j], i = 0..nxmap-1, is the reference's mapArray(nxmap,nymap): pixel i+1 along the sweep frame's first
 * axis, j+1 along its second; izone turns the sweep frame into storage as rotateIndices does (ftte_rotate_indices), for base
 * cells and for the children of a refined cell (the is/js/ks arrays of equiSources.f90:690-696).  The window is
 * [start, end] = [max(centre - 0.5/zoom, 0), min(start + 1/zoom, 1)] on each map axis (:685-689). */

/* The per-column (or per-row) quantities of the driver's pixel loops, equiSources.f90:703-709: base[i-1] = i0 (1-based base
 * cell) and frac[i-1] = xnew (position inside it) for x0 = (end-start)*(float(i)-0.5)/float(nmap) + start, evaluated left to
 * right in double as the compiled line is.  Context-free, host only.  FTTE_ERR_ARG where an i0 would leave 1..n. */
int ftte_map_axis(int n, int nmap, double centre, double zoom, int32_t *base /*[nmap]*/, double *frac /*[nmap]*/);
/* The same for the reader's loops, readCellArray.f90:126-132, whose x0 is the single-precision quotient (float(i)-0.5)/float(nmap)
 * widened: x0 = (end-start)*quotient + start, which is the reader's own x0 for the whole box (centre 0.5, zoom 1; the reader
 * has no window).  It differs from ftte_map_axis in the last bits of xnew. */
int ftte_slice_axis(int n, int nmap, double centre, double zoom, int32_t *base /*[nmap]*/, double *frac /*[nmap]*/);
/* kstart and kend of the projection, :687-700: the base cells (1-based, inclusive) between max(centre - 0.5/zoom, 0) and
 * min(centre + 0.5/zoom, 1), clamped to 1..n. */
int ftte_map_depth(int n, double centre, double zoom, int32_t *kstart, int32_t *kend);

/* The slice map of the reader tool, readCellArray.f90:116-140 with sliceCell :189-230: every pixel is the value of the leaf that
 * holds (x0, y0, zslice), rounded to float32.  value[ncell] (host; _device: any device array of ncell doubles, e.g. one group of
 * a swept J or one plane of ftte_point_rates_device); NULL = HI of the medium, as in the reference.  Axes: ftte_slice_axis. */
int ftte_slice_map(ftte_ctx *ctx, int izone, int nxmap, int nymap, const double centre[2], double zoom, double zslice,
                   const double *value, float *map);
int ftte_slice_map_device(ftte_ctx *ctx, int izone, int nxmap, int nymap, const double centre[2], double zoom, double zslice,
                          const double *value_dev, float *map);
/* mode 0: the projection of mode initialConfiguration, equiSources.f90:678-719 with projectVariableToMap :4914-4954 (the
 * reference: izone 3, 1024^2, centre (.5,.5,.5), zoom 2): per pixel the leaves of base cells kstart..kend along the depth, both
 * depth children of every refined cell, accumulated as :4948-4950 -- a float32 pixel, widened and rounded for every leaf, a
 * double totalMass -- and divided at the end; a column of rho = 0 gives NaN, as there.  value NULL = abun2 of the medium.
 * mode 1 is NOT in the reference; it is this build's own definition: the path integral sum value * leaf size [cm] over the same
 * leaves in the same order (a column density where value is a number density), summed in double and rounded to float32 once.
 * Axes: ftte_map_axis and ftte_map_depth. */
int ftte_project_map(ftte_ctx *ctx, int izone, int nxmap, int nymap, const double centre[3], double zoom, int mode,
                     const double *value, float *map);
int ftte_project_map_device(ftte_ctx *ctx, int izone, int nxmap, int nymap, const double centre[3], double zoom, int mode,
                            const double *value_dev, float *map);
/* mode clumpingFactor, equiSources.f90:661-676 with computeClumping :4711-4735: volume = volSum, mean_nh = volSumDensity/volSum,
 * clumping = (volSumDensity2/volSum) / mean_nh**2, nh = psi*rho/mh.  The sums are the library's own fixed-order sums (as
 * ftte_hydrogen_mass): the same bits on every call, the reference's sequential sums to rounding.  Any output may be NULL. */
int ftte_clumping(ftte_ctx *ctx, double *clumping, double *volume, double *mean_nh);
/* pdfGas and pdfGasOutside of mode plotPDFs, equiSources.f90:814-822 with computeGasPDF :4682-4709: the volume (base cells) of
 * the leaves in each of the 50 bins of log10(rho/msun*pc**3) between -8 and 3, and of those outside (rho = 0 among them).
 * Counted as integers per bin and level on the device and weighed on the host, which is exact. */
int ftte_gas_pdf(ftte_ctx *ctx, double pdf[50], double *outside);
/* pdfStar, pdfStarOutside and meanHostDensity/float(nStarsSpecificAge) of :787-813 for the stars with weight > 0, which arrive as
 * their host leaves (ftte_locate_cell), as they do for the tracer: a gather of nsrc leaves.  mean_host_HI may be NULL. */
int ftte_star_pdf(ftte_ctx *ctx, int nsrc, const int64_t *src_cell, int32_t pdf[50], int32_t *outside, double *mean_host_HI);

/* ---- absorption spectra along sightlines: the optical depth of a line in velocity space ------------
 * Not in the reference (which carries the cell array's velocities and never reads them); this build's own definition, stated in
 * full in csrc/ftte_spectra_math.h.  Single-device context, as the analysis above.
 *
 * The velocity field: [ncell] doubles in cm/s each, cell-array order; velx runs along storage-i, vely along storage-j, velz along
 * storage-k, the tracer's frame (what ftte_cellarray_fields hands out).  Three NULLs drop the field; with no field the peculiar
 * velocity is zero.  The field has an owner of its own in the context (it is no field of the medium), is dropped by
 * ftte_set_grid with another grid and counts in ftte_counter("device_objects").  FTTE_ERR_STATE without a grid,
 * FTTE_ERR_UNSUPPORTED on a multi-device context, FTTE_ERR_ARG for one or two NULLs. */
int ftte_set_velocity(ftte_ctx *ctx, const double *velx, const double *vely, const double *velz);
int ftte_set_velocity_device(ftte_ctx *ctx, const double *velx_dev, const double *vely_dev, const double *velz_dev);
/* tau(v) of one line along every pixel column of ftte_project_map's map: the same axis tables (ftte_map_axis), the same depth
 * (ftte_map_depth), the same leaves in the same order -- base cells kstart..kend, both depth children of a refined cell, k = 1
 * before 2.  The line of sight is the sweep frame's depth axis: a leaf's velocity u is the component of the storage axis the depth
 * feeds, negated where izone mirrors it.
 *   line[4] = {sigma_line = (pi e^2 / m_e c) f lambda0 [cm^2 cm/s] (HI Lyman alpha: 1.3435e-7), damping = Gamma lambda0 / 4 pi
 *   [cm/s] (0: a pure Doppler profile), mass of the absorber [g], b_turb [cm/s]}.
 * Leaf l with path D_l (its size [cm]), density n_l = value (NULL: HI of the medium), temperature T_l (the context's:
 * ftte_set_temperature or what the thermal steps left): N_l = n_l D_l, b_l = sqrt(2 k_B T_l / mass + b_turb^2), a_l = damping / b_l,
 * v_l = hubble s_l + u_l with s_l [cm] the distance of the leaf's centre from the entry face of base cell kstart.  Pixel p at
 * v_p = v0 + (p + 1/2) dv, d = v_p - v_l reduced by period rint(d / period) where period > 0, x = d / b_l:
 *   tau_p = sum_l N_l sigma_line / (sqrt(pi) b_l) H(a_l, x),  leaves in sightline order, one running sum per pixel,
 * H Tepper-Garcia's (2006) approximation of the Voigt function (exp(-x^2) exactly 0 for x^2 > 64; its error: DESIGN.md 8).
 *   tau[(i + nxmap j) nvel + p];  summary[(i + nxmap j) 3 + {0, 1, 2}] = N = sum N_l (float32(N) is ftte_project_map's mode-1
 *   pixel), W = sum_p (1 - exp(-tau_p)) dv, dv90 = (p_hi - p_lo) dv with p_lo, p_hi the first pixels whose running sum of tau
 *   reaches 0.05 and 0.95 of the total (0 where the total is 0).
 * Either output may be NULL (not both).  _device: value_dev, tau_dev and summary_dev are device pointers.  The same bits call
 * after call (no floating-point atomics).  Working memory belongs to the context; sightlines go in batches so that it stays
 * under 64 MiB (beyond that only where a single line needs more).
 * Refusals: as the maps'; FTTE_ERR_ARG for nvel < 1, dv <= 0, mass <= 0, a negative damping, b_turb or period, anything not finite;
 * FTTE_ERR_STATE without a temperature; FTTE_ERR_ARG where 2 k_B T / mass + b_turb^2 of any leaf on a sightline is not positive and
 * finite, decided in a pass of its own before anything of the caller's is written: on a refusal the outputs are untouched.
 * ftte_counter: "spectra_chunk_segments" (segments of a sightline held in LDS at a time), "spectra_pass_pixels" (pixels of a
 * sightline a workgroup holds in registers in one pass), "spectra_velocity" (1: a field is set). */
int ftte_sightline_spectra(ftte_ctx *ctx, int izone, int nxmap, int nymap, const double centre[3], double zoom, int nvel, double v0,
                           double dv, double hubble, double period, const double line[4], const double *value, double *tau,
                           double *summary);
int ftte_sightline_spectra_device(ftte_ctx *ctx, int izone, int nxmap, int nymap, const double centre[3], double zoom, int nvel,
                                  double v0, double dv, double hubble, double period, const double line[4], const double *value_dev,
                                  double *tau_dev, double *summary_dev);
/* The same line along rays of any origin and direction (the walk is stated in full in csrc/ftte_ray_math.h).  Frame and units: the
 * storage frame of ftte_set_velocity (x along storage-i, y along j, z along k), lengths in base cells: the box is [0, n]^3.
 *   origin[nray][3], dir[nray][3] the caller's unit vectors (| |dir|^2 - 1 | <= 1e-9), tmax[nray] the rays' ends in base cells from
 *   their origins, or NULL; a tmax <= 0 means "to the box's far side".  A ray starts where it enters the box, or at its origin inside.
 * The ray's leaves in the order it crosses them, each with its chord: leaf l has D_l = chord cell size [cm], s_l [cm] the distance
 * of the chord's midpoint from the ray's origin, u_l = (d_0 velx + d_1 vely) + d_2 velz.  Everything else is as above:
 *   tau[r nvel + p];  summary[3 r + {0, 1, 2}] = N, W, dv90.
 * A ray along +-e_a from a base cell's face through dyadic transverse coordinates equals the matching pixel column of
 * ftte_sightline_spectra bit for bit.  A ray that misses the box is no error: N = 0, tau = 0, W = 0, dv90 = 0.  The rays are host
 * arrays in both variants; _device: value_dev, tau_dev and summary_dev are device pointers.  Rays go in batches so that their
 * segment records and staged tau stay under 64 MiB (beyond that only where a single ray needs more); the same bits call after call.
 * Refusals: those of ftte_sightline_spectra; FTTE_ERR_ARG for nray < 1, an origin, direction or tmax that is not finite, a
 * direction that is no unit vector; FTTE_ERR_UNSUPPORTED on a multi-device context or a tree deeper than 40 levels;
 * FTTE_ERR_INTERNAL where a walk took more than 3 n 2^maxlevel + 3 steps.  All decided, the leaves' line widths included, before
 * anything of the caller's is written: on a refusal the outputs are untouched.  These three calls end a ray at the box's far side;
 * their _periodic namesakes below wrap it through the opposite face.  A leaf has one velocity.
 * ftte_counter: "ray_chunk_segments" (records of a ray held in LDS at a time), "ray_work_bytes" (the budget of a batch). */
int ftte_ray_spectra(ftte_ctx *ctx, int64_t nray, const double *origin, const double *dir, const double *tmax, int nvel, double v0,
                     double dv, double hubble, double period, const double line[4], const double *value, double *tau, double *summary);
int ftte_ray_spectra_device(ftte_ctx *ctx, int64_t nray, const double *origin, const double *dir, const double *tmax, int nvel,
                            double v0, double dv, double hubble, double period, const double line[4], const double *value_dev,
                            double *tau_dev, double *summary_dev);
/* The rays' segment lists: ray r's segments are offset[r] .. offset[r + 1] - 1 (offset[nray + 1]), each the leaf's cell-array index
 * and its [t_in, t_out] in base cells from the ray's origin; a ray's segments tile [its start, its end] without a gap.  Needs a
 * grid only.  capacity: the room of leaf, t_in and t_out; 0 returns the offsets alone (the three may be NULL), a capacity below
 * offset[nray] is FTTE_ERR_ARG with everything untouched. */
int ftte_ray_segments(ftte_ctx *ctx, int64_t nray, const double *origin, const double *dir, const double *tmax, int64_t *offset,
                      int64_t capacity, int64_t *leaf, double *t_in, double *t_out);
/* Periodic rays: the box tiles space with period n on every axis and a ray goes on through the box's opposite face (the statement is
 * in csrc/ftte_ray_math.h).  The arguments are those of the namesakes above, except that tmax[nray] is required and every entry is
 * the ray's length in base cells, finite and > 0: a periodic ray always hits, runs from t = 0 at its origin (any finite point, in
 * the box or not) to t = tmax, and its segments tile [0, tmax].  t and s_l are measured from the caller's origin along the whole ray,
 * across images, so the Hubble velocity keeps growing; `period` folds velocities as before, not positions.  A ray along +-e_a of
 * length k n from a base cell's face gives the one-box list k times with t shifted by exactly j n; a ray that ends before its first
 * wrap equals the non-periodic ray of that tmax bit for bit.  Refusals beyond the namesakes': FTTE_ERR_ARG for tmax == NULL or a
 * tmax <= 0 (the message names the first such ray); FTTE_ERR_UNSUPPORTED for a tmax above 2^20 boxes, an origin more than 2^20
 * boxes away or a step bound 3 (n 2^maxlevel) (ceil(tmax / n) + 1) + 3 beyond 2^62, the reason in the message. */
int ftte_ray_spectra_periodic(ftte_ctx *ctx, int64_t nray, const double *origin, const double *dir, const double *tmax, int nvel, double v0,
                              double dv, double hubble, double period, const double line[4], const double *value, double *tau,
                              double *summary);
int ftte_ray_spectra_periodic_device(ftte_ctx *ctx, int64_t nray, const double *origin, const double *dir, const double *tmax, int nvel,
                                     double v0, double dv, double hubble, double period, const double line[4], const double *value_dev,
                                     double *tau_dev, double *summary_dev);
int ftte_ray_segments_periodic(ftte_ctx *ctx, int64_t nray, const double *origin, const double *dir, const double *tmax, int64_t *offset,
                               int64_t capacity, int64_t *leaf, double *t_in, double *t_out);

/* ---- host arrays ------------------------------------------------------------------------------
 * The reference keeps its fields in host memory (the zoneType tree, definitionsModule.f90:163-180); the drop-ins
 * flatten them into cell-array order and hand them over.  Pageable arrays cross PCIe through pinned staging blocks
 * inside the library; an array registered here is pinned in place and moved by DMA directly, for as long as it stays
 * registered (the caller unregisters it before freeing it).  bytes counts from ptr. */
int ftte_host_register(ftte_ctx *ctx, void *ptr, size_t bytes);
int ftte_host_unregister(ftte_ctx *ctx, void *ptr);

/* ---- tuning and instrumentation ------------------------------------------------------------- */

/* How often the expensive host-side builds have run on this context: "grid_builds" (tree rebuilt from a level list:
 * ftte_set_grid with an unchanged list keeps the tree, the plans and the resident medium), "plan_builds" (tiled-sweep
 * planner), "forest_builds" (per-direction segment forests of a refined cell array); of the hybrid sweep's current plan, "hybrid_boxes"
 * (boxes around clusters of refined cells, of the izone that has most) and "hybrid_passes" (passes their forests are swept in), 0
 * when the last sweep did not take the hybrid path; "fine_block": fine cells a side of the refined block that plan sweeps with bricks of
 * its own (0: none); "brick_form": the form of the brick kernel the last uniform-grid sweep of the
 * brick engine took (option "team": 0 or 2; -1 before the first); "brick_dataflow": how that sweep was launched (0 a launch per
 * stage, 1 one launch with flags, 2 the same with write-through stores, 3 persistent workgroups with a queue per XCD; the form
 * option "dataflow" asks for falls back to 1 or 0 where the XCD census or the grid size does not allow it; -1 before the first);
 * "brick_whole": 1 when that sweep's stage launches took the whole-brick form of the brick kernel (every brick whole, four waves, no
 * emission, no diagnostic option), else 0; "brick_duo": the workgroups per stage sweep of that sweep's plan in which two passes of one
 * izone cross a brick together and share its opacities and its J (0: every pass on its own); "nu_deal": option "nu_deal" as it stands (the library's default until it is set);
 * "brick_groups" and "brick_accumulators" (also "_0", "_1", "_2" per memory layout): direction groups of the current brick plan and
 * the J accumulators they share (0 without a plan), "brick_chunk" (layers per brick of that plan) and "brick_queue_mix" (the
 * option "queue_mix" the persistent form's queues were laid out by; -1 when the plan has no queues); "brick_stages" (stages of that
 * plan), "merge_points" and "merge_blocks" (its block-wise merge: points and 32^3-cell blocks), "merge_stage_K" and "merge_final_K"
 * (the stage after which point K runs, the blocks final by then); "expansion_exact_tests" (ftte_expand_hii_regions);
 * "catalogue_stars" and "catalogue_sources" (the stars and the sources of the last ftte_star_catalogue; -1 sources: there is none),
 * "catalogue_ns_locate", "_count", "_scan", "_emit" (device time of that call's four launches in nanoseconds, from events recorded
 * around them; -1 where the launch did not run), "medium_abun2" (1: the medium of ftte_set_medium came with an abun2); "devices"; of a multi-device context also "frequency_slices",
 * "direction_slices" and "multi_rccl" (1: the last direction-split sweep was summed over RCCL), "rccl_loadable", "rccl_selftest" (runs the
 * direction sum's RCCL calls on a clique of one rank, the first device: 1 = the piece came back unchanged; negative = it could not
 * run), the rest from its first device.
 * "device_objects": device buffers, pinned buffers, streams, events and captured graphs the library holds at the moment, over all
 * contexts of the process (single- and multi-device contexts alike): what a destroyed context had made is no longer in it.
 * -1 for an unknown name. */
long long ftte_counter(const ftte_ctx *ctx, const char *name);

/* Tuning knobs.  0 means automatic where noted.  Every option belongs to the context it is set on.  Results do not depend on any of them except through the order in which the
 * directions' contributions are added into J (last bits); unknown keys return FTTE_ERR_ARG.
 *   uniform grids
 *     "engine"      0 automatic = 2 cell-fixed bricks, 1 ray-following tiles (3a)
 *     "chunk"       bricks: layers per brick (0: 16, fewer with few frequency groups)
 *     "group"       bricks: most directions of one izone that share a brick pass, 1..8 (0: 3)
 *     "share"       bricks: groups sharing a J accumulator: 0 none, 1 the passes of one izone, 2 and izone pairs (default)
 *     "lanes"       bricks: streams the frequency groups (or, with fewer groups than lanes, the direction groups) are spread over
 *     "brick_waves" bricks: waves per SIMD the kernel is compiled for, 2..4
 *     "dataflow"    bricks: 0 a launch per stage, 1 one launch whose bricks wait for each other, 2 the same with
 *                   write-through stores, 3 one launch of persistent workgroups with a task queue per XCD
 *     "tiled"       bricks: 1 = opacities and accumulators stored brick by brick (a brick's layer in one piece; grids of whole
 *                   bricks), 2 = the whole brick in one piece; same results, measured without gain; 0 = in frames (default)
 *     "nu_deal"     bricks, a launch per stage: how a launch's workgroups are dealt to its (brick, frequency group) pairs.  0:
 *                   workgroup b sweeps group b mod nnu, so each group always runs on the same XCDs; K >= 1: the groups are turned
 *                   by one after every run of K bricks per XCD round, so every XCD sweeps every group equally often.
 *                   Same results bit for bit; no plan depends on it.  0..4096, default 16 (1 puts every group's opacities behind
 *                   every L2 and gains nothing with two streams; 4 to 64 measured alike)
 *     "merge_overlap" bricks: 1 (default) = J merged block by block (32^3 cells) while the last stages run, 0 = one merge after
 *                   the last stage; same results
 *     "team"        bricks: 0 = one wavefront per brick, 2 = two wavefronts per brick, four rows each; -1 (default): 2 with up to
 *                   four frequency groups on this GPU, else 0
 *     "pair_waves"  bricks, two wavefronts per brick: workgroups per SIMD that form is compiled for, 2..4
 *     "rows", "stack", "slots", "waves"  tiles: rays per lane (4, 8, 16), wavefronts per workgroup (1, 2, 4, 8), directions in flight
 *                   per launch (1..16), waves per SIMD (2..6); built variants rows x stack = 4x{1,4,8}, 8x{1,2,4}, 16x1
 *   refined cell arrays
 *     "hybrid"      1 bricks outside boxes around the refined cells, segment forests inside (default; 3b), 0 forests for the whole tree
 *     "hybrid_slots" hybrid: where the bricks' launches go around the passes of the forests: 0 = phases (a phase of brick stages per
 *                   pass), 1 (default) = slots where there are several passes (every brick in the earliest launch its own inputs
 *                   allow), 2 = slots always
 *     "pipelines"   hybrid: independent bricks-forests-bricks sequences on streams of their own, 1..4 (default 3)
 *     "box_lanes"   hybrid: along a brick's 64 lanes the boxes end on multiples of this (a divisor of 64; default 1: one cell beyond
 *                   the refined cells)
 *     "graph"       hybrid: 1 = the launches of a sweep are captured once into a hipGraph and replayed (default 0: measured slower
 *                   than issuing them on this runtime)
 *     "fine_bricks" hybrid: 1 (default) = a fully refined block -- one cluster that is a cube of base cells refined exactly once, twice
 *                   its side a multiple of 64 -- is swept by bricks of its own on the fine level, the forests keep what lies around it
 *                   (DESIGN.md 3b); 0 = every leaf of a box through the forests.  "fine_chunk": layers per fine brick (0: as "chunk")
 *     "forest_batch" most directions per launch of the segment forests (0: what the path and the device memory allow)
 *     "forest_fuse" runs of forest levels with at most this many (segment, frequency group) pairs in the fullest direction go in ONE
 *                   launch, a workgroup per direction and a barrier per level (default 4096; 0: a launch per level).  Same bits.
 *     "forest"      1: use the segment forests on a uniform grid too, for cross-checks
 *   "ldspad"        diagnostic, per context like every option: extra dynamic LDS per workgroup of this context's sweep launches
 *                   (bytes, 0..163840), to cap residency
 *   "atomic_acc"    bricks: 1 = later visitors of a shared accumulator add with fp64 atomics instead of read-add-store (default 0)
 *   "queue_mix"     bricks, dataflow = 3: how (frequency group, accumulator) units are dealt to the XCDs' queues: 0 a frequency
 *                   group per queue where they divide, 1 by load, 2 (group + accumulator) mod queues
 *   "ablate"        diagnostic, WRONG RESULTS, timing only: mask of parts of the brick kernel's memory traffic to leave out
 *   multi-device contexts: every option goes to every device; "multi_reduce" 1 = always sum direction slices with the peer kernel */
int ftte_set_option(ftte_ctx *ctx, const char *key, int value);
/* Launch records of the last sweep (valid after the sweep's stream has been synchronised).
 * Each sweep-kernel launch is bracketed by HIP events on the stream it runs on. */
int ftte_launch_count(const ftte_ctx *ctx);
/* ms: device time of launch `idx`; updates: cell.direction.frequency updates it performed. */
int ftte_launch_info(ftte_ctx *ctx, int idx, double *ms, int64_t *updates);

/* ---- host geometry, the reference's callable surface (no device needed) ---------------------- */

/* one layer's ray pattern: patternType of definitionsModule.f90:141-152 without the tree link */
typedef struct {
    double xy_x0, xy_y0, xy_len;
    double xz_x0, xz_z0, xz_len;
    double yz_y0, yz_z0, yz_len;
    int32_t xz_active, yz_active;
    int32_t xy_top, xz_top, yz_top; /* 0 none, 1 xy segment, 2 yz segment, 3 xz segment (:159) */
    int32_t reserved_;
} ftte_pattern;

/* rotateIndices(i,j,k,nx,ny,nz,izone,icell,jcell,kcell), rotateIndicesModule.f90:7-113 */
int ftte_rotate_indices(int i, int j, int k, int nx, int ny, int nz, int izone, int *icell, int *jcell, int *kcell);
/* pix2ang_nest + rotateAngles, equiSources.f90:2118-2231, 2297-2335: rotated centre of NESTED
 * pixel ipix; phi in [0, 2 pi), theta = colatitude - pi/2 */
int ftte_pix2ang_nest(int nside, int64_t ipix, double *phi, double *theta);
/* direction folding, equiSources.f90:1395-1454: canonical (phi, theta) and izone 1..24 */
int ftte_fold_direction(double phi_large, double theta_large, double *phi, double *theta, int *izone);
/* setPattern(pattern, phi, theta), transportRoutinesModule.f90:7-85; xy_x0, xy_y0 are inputs */
int ftte_set_pattern(ftte_pattern *pattern, double phi, double theta);
/* patterns of layers 1..n of a folded direction, equiSources.f90:1495-1534 */
int ftte_layer_patterns(int n, double phi, double theta, ftte_pattern *layers);
/* computeCellIntensity(Jmean, Iin, Iout), transportRoutinesModule.f90:1036-1054 */
void ftte_compute_cell_intensity(double *Jmean, double Iin, double Iout);

#ifdef __cplusplus
}
#endif
#endif /* FTTE_H */
