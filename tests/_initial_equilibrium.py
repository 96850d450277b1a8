"""A numpy restatement of the start-up ionisation equilibrium and of computeMass (equiSources.f90:3679-3868, :4369-4393,
:5044-5058): the yardstick of ftte_initial_ionization_equilibrium and ftte_hydrogen_mass.

Every operation is a plain IEEE binary64 add, multiply or divide in the reference's order (numpy rounds each one on its own);
the logarithm of the temperature is the host's libm log, as ftte_set_temperature takes it.  All cells bisect in lockstep, each
stopping where the reference's `do while (HeI .ne. HeIprev)` would.
"""
import math

import numpy as np

F32 = lambda x: float(np.float32(x))  # noqa: E731  (a default-real literal widened)
PSI, MP, MN = F32(0.76), F32(1.6726231e-24), F32(1.67492728e-24)
MH, MHE, PI, MSUN = MP, 2.0 * (MP + MN), F32(3.141592654), F32(1.98892e33)
MAX_STEPS = 4096


def logtem_of(tgas):
    return np.array([math.log(t) for t in np.asarray(tgas, np.float64)])


def rate_coefficients(logtem, logtem0, logtem9, dlogtem, k):
    """k1..k6 interpolated in log T (:3747-3766)"""
    k = np.asarray(k, np.float64)
    nratec = k.shape[1]
    lt = np.fmin(np.fmax(logtem, logtem0), logtem9)
    ix = ((lt - logtem0) / dlogtem).astype(np.int64) + 1
    ix = np.minimum(nratec - 1, np.maximum(1, ix))
    t1 = logtem0 + (ix - 1).astype(np.float64) * dlogtem
    t2 = logtem0 + ix.astype(np.float64) * dlogtem
    tdef = t2 - t1
    return [k[r, ix - 1] + (lt - t1) * (k[r, ix] - k[r, ix - 1]) / tdef for r in range(6)]


def _residual(kk, kr24, kr25, kr26, nh, nhe, de):
    k1, k2, k3, k4, k5, k6 = kk
    X = k3 * de + kr26
    Y = k4 * de
    HII = nh / (1.0 + k2 * de / (k1 * de + kr24))
    HeI = (de - HII - 2.0 * nhe) / (X / Y - 2.0 - 2.0 * X / Y)
    HeII = HeI * X / Y
    res = k3 * HeI * de + k6 * (nhe - HeI - HeII) * de + kr26 * HeI - HeII * (k4 * de + k5 * de + kr25)
    return res, HeI


def initial_pass(rho, HI0, HeI0, HeII0, kk, uniform, threshold):
    """one initialIonizationEquilibrium per cell: (HI, HeI, HeII, steps, ok)"""
    with np.errstate(all="ignore"):
        nh = PSI * rho / MH
        nhe = (1.0 - PSI) * rho / MHE
        HI = np.fmin(HI0, nh)
        HeI = HeI0.copy()
        HeII = np.where((nhe - HeI0 - HeII0 < 0.0) & (nhe - HeI0 < 0.0), 0.0, HeII0)
        mfp = 1.0 / (HI * F32(6.3e-18) + HeI * F32(7.42e-18) + HeII * F32(1.58e-18))
        lit = mfp >= threshold
        kr24, kr25, kr26 = (np.where(lit, 4.0 * PI * uniform[g], 0.0) for g in range(3))
        de1 = np.full_like(rho, F32(1.e-20))
        de2 = nh + 2.0 * nhe
        res1, HeI = _residual(kk, kr24, kr25, kr26, nh, nhe, de1)
        _, HeI = _residual(kk, kr24, kr25, kr26, nh, nhe, de2)
        de = de2.copy()
        HeIprev = np.full_like(rho, -1.0)
        steps = np.zeros(rho.shape, np.int64)
        active = HeI != HeIprev
        while active.any() and steps.max() < MAX_STEPS:
            a = np.nonzero(active)[0]
            HeIprev[a] = HeI[a]
            d = 0.5 * (de1[a] + de2[a])
            de[a] = d
            res, h = _residual([x[a] for x in kk], kr24[a], kr25[a], kr26[a], nh[a], nhe[a], d)
            HeI[a] = h
            r1 = res1[a]
            opp = ((res > 0.0) & (r1 < 0.0)) | ((res < 0.0) & (r1 > 0.0))
            de2[a] = np.where(opp, d, de2[a])
            de1[a] = np.where(opp, de1[a], d)
            steps[a] += 1
            active[a] = HeI[a] != HeIprev[a]
        HIprev = np.where(steps > 0, HI, -1.0)
        HeIIprev = np.where(steps > 0, HeII, -1.0)
        converged = (HeI == HeIprev) & ~(HIprev != HI) & ~(HeIIprev != HeII)
        k1, k2, k3, k4 = kk[:4]
        X = k3 * de + kr26
        Y = k4 * de
        HII = nh / (1.0 + k2 * de / (k1 * de + kr24))
        HI = k2 * HII * de / (k1 * de + kr24)
        ok = converged & (HI / nh >= 0.0) & (HI / nh <= 1.0) & (HeI / nhe >= 0.0) & (HeI / nhe <= 1.0)
        HeII = HeI * X / Y
    return HI, HeI, HeII, steps, ok


def initial_equilibrium(rho, tgas, HI, HeI, HeII, uniform, threshold, logtem0, logtem9, dlogtem, k, passes=2):
    """`passes` passes per cell: (HI, HeI, HeII, steps per pass [passes][ncell], ok); a cell that fails keeps failing"""
    rho = np.asarray(rho, np.float64)
    kk = rate_coefficients(logtem_of(tgas), logtem0, logtem9, dlogtem, k)
    state = [np.array(a, np.float64) for a in (HI, HeI, HeII)]
    ok = np.ones(rho.shape, bool)
    steps = []
    for _ in range(passes):
        *state, s, good = initial_pass(rho, *state, kk, np.asarray(uniform, np.float64), threshold)
        ok &= good
        steps.append(s)
    return state[0], state[1], state[2], np.array(steps), ok


def mass_terms(n, level, box, HI, rho):
    """computeMass per leaf: (HI mh cs3 / msun, psi rho cs3 / msun) with cs3 the cube of box/(float(2**level) float(n))"""
    lev = np.asarray(level, np.int64)
    size = box / ((2.0 ** lev).astype(np.float32) * np.float32(n)).astype(np.float64)
    cs3 = size * size * size
    return np.asarray(HI, np.float64) * MH * cs3 / MSUN, PSI * np.asarray(rho, np.float64) * cs3 / MSUN


def hydrogen_mass(n, level, box, HI, rho):
    """the two sums, exactly rounded (math.fsum): what a sum in any order approaches"""
    neutral, total = mass_terms(n, level, box, HI, rho)
    return math.fsum(neutral), math.fsum(total)
