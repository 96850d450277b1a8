"""The oracle against the reference: every vector under tests/golden/ was produced by the reference's own
compiled modules (oracle/_ref/ref_harness, tests/golden/make_golden.py); the C restatement must reproduce
them.  Plus the known-answer tests SURVEY.md section 8(c) asks for, since the reference ships no tests."""
import numpy as np
import pytest

import _oracle as O

EPS = np.finfo(np.float64).eps


def test_rotate_indices_table(golden):
    g = golden("rotate_indices")
    nx, ny, nz = map(int, g["extents"])
    t = g["table"]
    for z in range(24):
        for i in range(3):
            for j in range(4):
                for k in range(5):
                    assert O.rotate_indices(i + 1, j + 1, k + 1, nx, ny, nz, z + 1) == tuple(t[z, i, j, k])


@pytest.mark.parametrize("name", ["geometry_192dir_16layers", "geometry_12dir_256layers"])
def test_fold_and_patterns_bitwise(golden, name):
    g = golden(name)
    n = int(g["n"])
    for d in range(len(g["phi_in"])):
        p, t, z = O.fold_direction(g["phi_in"][d], g["theta_in"][d])
        assert (p, t, z) == (g["phi"][d], g["theta"][d], g["izone"][d])
        L = O.layer_patterns(n, p, t)
        for i in range(n):
            r, P = g["layers"][d][i], L[i]
            assert (P.xz_active, P.yz_active, P.xy_top, P.xz_top, P.yz_top) == tuple(r["flags"])
            assert (P.xy_x0, P.xy_y0, P.xy_len) == tuple(r["xy"])
            if P.xz_active:
                assert (P.xz_x0, P.xz_z0, P.xz_len) == tuple(r["xz"])
            if P.yz_active:
                assert (P.yz_y0, P.yz_z0, P.yz_len) == tuple(r["yz"])


UNIFORM = ["uniform8_transparent", "uniform16_constant", "uniform16_lognormal_24zones", "uniform24_lognormal_48dir"]
AMR = ["amr8_block_level1", "amr6_scattered_level2"]


def _args(g):
    return (g["kappa"], float(g["box"]), g["phi"], g["theta"], g["w"], g["uvb"])


@pytest.mark.parametrize("name", UNIFORM)
def test_uniform_sweep_bitwise(golden, name):
    g = golden(name)
    J = O.sweep_uniform(int(g["n"]), *_args(g))
    assert np.array_equal(J, g["J"])


@pytest.mark.parametrize("name", UNIFORM + AMR)
def test_tree_sweep_bitwise(golden, name):
    g = golden(name)
    J = O.sweep_tree(int(g["n"]), g["level"], *_args(g))
    assert np.array_equal(J, g["J"])


@pytest.mark.parametrize("name", UNIFORM)
def test_device_arithmetic_within_reference_noise(golden, name):
    """The identity log(Iin/Iout) == tau used on the device differs from the reference formula only by the
    reference's own rounding noise, bounded per cell by the oracle (see ftte_oracle.h: noise)."""
    g = golden(name)
    n = int(g["n"])
    J, noise = O.sweep_uniform(n, *_args(g), with_noise=True)
    Jd = O.sweep_uniform(n, *_args(g), arith=O.ARITH_DEVICE)
    assert np.all(np.abs(Jd - J) <= 8 * noise + 12 * n * EPS * np.abs(J))


def config1_case(golden):
    """BASELINE configs[0]: 64^3 uniform, 1 frequency group, 6 directions through izones 1, 2, 3, 13, 14, 15; the opacity field is
    regenerated from the seed the golden file names (first of three generated groups)."""
    from radiativetransfer_amd import synthetic
    g = golden("config1_uniform64_6dir")
    n = int(g["n"])
    kappa, uvb, box = synthetic.uniform_workload(n, int(g["nnu_generated"]), seed=int(g["seed"]), tau_median=float(g["tau_median"]))
    assert box == float(g["box"]) and np.array_equal(uvb[:1], g["uvb"])
    return g, n, np.ascontiguousarray(kappa[:1]), box


def test_config1_plumbing_case_bitwise(golden):
    """The reference's own driver lines (lifted, inline base-cell branch) on the config-1 workload: the oracle reproduces J
    bit for bit, all six directions land in the izones the survey names."""
    g, n, kappa, box = config1_case(golden)
    assert [O.fold_direction(p, t)[2] for p, t in zip(g["phi"], g["theta"])] == [1, 2, 3, 13, 14, 15] == list(g["izone"])
    J = O.sweep_uniform(n, kappa, box, g["phi"], g["theta"], g["w"], g["uvb"])
    assert np.array_equal(J, g["J"])


def test_lifted_driver_and_restated_driver_agree(golden):
    """oracle/_ref/ref_harness has two routes through a direction: the reference's own driver lines lifted from
    equiSources.f90:1393-1801 (what every golden is made with), and ref_harness.f90's own sequence of the same steps.  Same
    bits, on a uniform and on a refined cell array: both routes' J as the harness gave them (tests/golden/driver_routes.npz,
    tests/golden/make_golden_routes.py), and -- wherever the harness binary has been built -- as it gives them again."""
    import os
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
    import make_golden_routes as R
    g = golden("driver_routes")
    phi, theta, w, uvb = R.directions()
    assert all(np.array_equal(a, g[k]) for a, k in ((phi, "phi"), (theta, "theta"), (w, "w"), (uvb, "uvb")))
    live = os.path.exists(R.M.HARNESS)
    for c, (n, level, kappa) in enumerate(R.cases()):
        assert n == int(g[f"n{c}"]) and np.array_equal(level, g[f"level{c}"]) and np.array_equal(kappa, g[f"kappa{c}"])
        out = [g[f"J{c}_lifted"], g[f"J{c}_restated"]]
        if live:
            assert np.array_equal(R.run(n, level, kappa, True), out[0]) and np.array_equal(R.run(n, level, kappa, False), out[1])
        assert np.array_equal(out[0], out[1])
        assert np.array_equal(out[0], O.sweep_tree(n, level, kappa, R.BOX, phi, theta, w, uvb))


def test_transparent_box_gives_inflow(golden):
    g = golden("uniform8_transparent")
    assert np.allclose(g["J"], (g["uvb"] * g["w"].sum())[:, None], rtol=4 * EPS, atol=0)


def test_segment_lengths_sum_to_chord():
    """checkPattern's invariant (transportRoutinesModule.f90:258): a layer's pieces add up to 1/sin(theta)."""
    phi, theta, _ = O.healpix_directions(3)
    for p, t in zip(phi, theta):
        pf, tf, _ = O.fold_direction(p, t)
        for P in O.layer_patterns(48, pf, tf):
            total = P.xy_len + (P.xz_len if P.xz_active else 0) + (P.yz_len if P.yz_active else 0)
            assert abs(total * np.sin(tf) - 1) < 1e-12


def test_healpix_set_properties():
    """HEALPix NESTED centres (published algorithm, Gorski et al. 2005): nside = 1 rings sit at z = 2/3, 0, -2/3
    before the reference's fixed tilt; the tilt is a rotation, so pairwise angles are preserved and the set still
    averages to zero."""
    for level in (1, 2, 3):
        phi, theta, w = O.healpix_directions(level)
        assert abs(w.sum() - 1) < 1e-14
        v = np.stack([np.cos(theta) * np.cos(phi), np.cos(theta) * np.sin(phi), np.sin(theta)], 1)
        assert np.abs(v.sum(0)).max() < 2e-7 * len(phi)  # float32-rounded pi in the reference limits this
        assert np.all((phi > 0) & (phi < O.lib().fo_two_pi()))
    # un-tilt the 12 base pixels and compare with the analytic ring heights
    phi, theta, _ = O.healpix_directions(1)
    v = np.stack([np.cos(theta) * np.cos(phi), np.cos(theta) * np.sin(phi), np.sin(theta)], 1)
    a, b = np.float64(np.float32(0.111)), np.float64(np.float32(0.222))
    # rotateAngles tilts about x by a then about y by b (equiSources.f90:2305-2323); invert
    Ry = np.array([[np.cos(b), 0, -np.sin(b)], [0, 1, 0], [np.sin(b), 0, np.cos(b)]])
    Rx = np.array([[1, 0, 0], [0, np.cos(a), -np.sin(a)], [0, np.sin(a), np.cos(a)]])
    best = None
    for sy in (1, -1):
        for sx in (1, -1):
            Ryy, Rxx = (Ry if sy > 0 else Ry.T), (Rx if sx > 0 else Rx.T)
            z = (v @ Ryy.T @ Rxx.T)[:, 2]
            err = np.abs(np.sort(np.abs(z)) - np.sort(np.abs(np.array([2 / 3] * 4 + [0] * 4 + [-2 / 3] * 4)))).max()
            best = err if best is None else min(best, err)
    # theta = acos(z) - halfPi with the float32 pi: |z| = 2/3 or 0 up to that literal's 8.7e-8 error
    assert best < 1e-6


def test_constant_opacity_straight_chain():
    """A cell fed only through xy pieces of single-piece layers sees I = uvb exp(-kappa Delta n / sin theta)."""
    n, kap, box = 12, 3.0, 1.0
    # a steep direction: every layer single-piece for the first few layers at the cell centre
    phi, theta = 0.3, 1.45
    pf, tf, z = O.fold_direction(phi, theta)
    L = O.layer_patterns(n, pf, tf)
    depth = 0
    while depth < n and not (L[depth].xz_active or L[depth].yz_active):
        depth += 1
    assert depth >= 3
    uvb = np.array([1e-21])
    J = O.sweep_uniform(n, np.full((1, n ** 3), kap), box, [phi], [theta], [1.0], uvb)
    # cell in layer `m` (1-based) far from inflow faces other than the bottom
    delta = box / n
    for m in range(1, depth + 1):
        tau_seg = kap * delta / np.sin(tf)
        Iin = uvb[0] * np.exp(-tau_seg * (m - 1))
        expect = Iin * (1 - np.exp(-tau_seg)) / tau_seg
        i, j, k = m, n // 2, n // 2
        ic, jc, kc = O.rotate_indices(i, j, k, n, n, n, z)
        got = J[0, ((ic - 1) * n + (jc - 1)) * n + (kc - 1)]
        assert abs(got / expect - 1) < 1e-11


def test_cube_symmetry_permutes_J():
    """Rotating the opacity field by a cube symmetry and the direction with it permutes J (exercises every izone):
    here the 4-fold rotation about the polar axis, phi -> phi + pi/2, (x,y) -> (-y, x)."""
    n = 10
    rng = np.random.default_rng(3)
    kap = rng.lognormal(0, 1, (1, n, n, n)) * 2.0
    phi, theta, w = O.healpix_directions(2)
    uvb = np.array([1e-21])
    J0 = O.sweep_uniform(n, kap.reshape(1, -1), 1.0, phi, theta, w, uvb).reshape(n, n, n)
    # storage (ic,jc,kc): izone 1 has march = ic = polar axis z, jc = y, kc = x (transportRoutinesModule.f90:295-317).
    # rotate by +90 deg about z: x' = -y, y' = x  =>  kappa'(z, y', x') = kappa(z, y = -x', x = y')
    kap_r = np.transpose(kap[0], (0, 2, 1))[:, :, ::-1]  # [z][y'=x][x'=-y]
    assert kap_r[2, 3, 4] == kap[0, 2, n - 1 - 4, 3]
    pi = O.lib().fo_pi()
    phi_r = np.mod(phi + 0.5 * pi, 2 * pi)
    J1 = O.sweep_uniform(n, np.ascontiguousarray(kap_r).reshape(1, -1), 1.0, phi_r, theta, w, uvb).reshape(n, n, n)
    J1_back = np.transpose(J1[:, :, ::-1], (0, 2, 1))
    assert np.allclose(J1_back, J0, rtol=1e-9, atol=0)


def test_slotted_order_matches_serial_within_rounding(golden):
    g = golden("uniform16_lognormal_24zones")
    a = O.sweep_uniform(int(g["n"]), *_args(g), arith=O.ARITH_DEVICE, order=O.ORDER_SERIAL)
    b = O.sweep_uniform(int(g["n"]), *_args(g), arith=O.ARITH_DEVICE, order=O.ORDER_CLASSED)
    assert np.allclose(a, b, rtol=32 * EPS, atol=0)


def test_opacities_follow_reference_order():
    rng = np.random.default_rng(0)
    HI, HeI, HeII = rng.random((3, 100))
    beta = rng.random((3, 5))
    k = O.compute_opacities(HI, HeI, HeII, beta)
    for g_ in range(5):
        assert np.array_equal(k[g_], HI * beta[0, g_] + HeI * beta[1, g_] + HeII * beta[2, g_])


# ---- emission (the reference's never-enabled eta term, and the build's source function) ----------------------------------

def _emitting_case():
    from radiativetransfer_amd import synthetic
    n = 12
    kappa, uvb, box = synthetic.uniform_workload(n, 2, seed=2, tau_median=0.5)
    phi, theta, w = O.healpix_directions(2)
    rng = np.random.default_rng(1)
    return n, kappa, uvb, box, phi, theta, w, rng.random(kappa.shape) * 2e-22, rng.random(kappa.shape) * 3e-21


def test_zero_emissivity_array_equals_no_emissivity_in_reference_arithmetic():
    """eta = 0 everywhere through the emission formula is the reference as shipped (nemi = 0., :673-678)."""
    n, kappa, uvb, box, phi, theta, w, _, _ = _emitting_case()
    a = O.sweep_uniform(n, kappa, box, phi, theta, w, uvb)
    b = O.sweep_uniform(n, kappa, box, phi, theta, w, uvb, eta=np.zeros_like(kappa))
    assert np.array_equal(a, b)


@pytest.mark.parametrize("which", ["eta", "src"])
def test_emission_device_arithmetic_within_reference_noise(which):
    """eta: the reference's own (disabled) emissivity term and its log-mean, transcribed from :656-676; src: the build's source
    function with the exact path mean (ftte_math.h: ftte_segment_source) against its straightforward evaluation with libm."""
    n, kappa, uvb, box, phi, theta, w, eta, src = _emitting_case()
    kw = dict(eta=eta) if which == "eta" else dict(src=src)
    Jr, noise = O.sweep_uniform(n, kappa, box, phi, theta, w, uvb, with_noise=True, **kw)
    Jd = O.sweep_uniform(n, kappa, box, phi, theta, w, uvb, arith=O.ARITH_DEVICE, **kw)
    assert np.all(np.abs(Jd - Jr) <= 8 * noise)
    assert np.max(noise / Jr) < 1e-8  # the bound is not vacuous


def test_radiative_equilibrium_is_a_fixed_point():
    """S = inflow everywhere: every segment returns Iout = Iin, J = inflow * sum(w).  The device arithmetic keeps this to
    rounding; the reference's (Iin-Iout)/log(Iin/Iout) does not (its quotient is rounded before the logarithm)."""
    n, kappa, uvb, box, phi, theta, w, _, _ = _emitting_case()
    S = np.repeat(uvb[:, None], n ** 3, 1)
    J = O.sweep_uniform(n, kappa, box, phi, theta, w, uvb, src=S, arith=O.ARITH_DEVICE)
    assert np.allclose(J, uvb[:, None] * w.sum(), rtol=64 * EPS, atol=0)
