"""SourceIteration(accelerate="diagonal" | "diagonal+ng"): the approximate-operator iteration with the exact diagonal of the
Lambda operator, and Ng's extrapolation on top -- same fixed point as the plain Lambda iteration, fewer iterations.

The yardstick of the convergence test is a restatement on the host (tests/_lambda_host.py): the same three schemes with the
oracle's sweep as the sweep and the diagonal from probing it -- nothing of the code under test."""
import numpy as np
import pytest

import _lambda_host as H
import _oracle as O
import radiativetransfer_amd as rt
from radiativetransfer_amd import synthetic
from radiativetransfer_amd.iteration import SourceIteration

pytestmark = pytest.mark.gpu

EPS = np.finfo(np.float64).eps
SCHEMES = (None, "diagonal", "diagonal+ng")


def numpy_update(S, J, B, diag, eps):
    om = 1.0 - eps
    return S + (((om * J) + (eps * B)) - S) / (1.0 - (om * diag))


@pytest.mark.parametrize("b_per_cell", [False, True])
def test_update_kernel_against_its_numpy_statement(b_per_cell):
    import torch
    n, nnu, eps = 20, 3, 1e-2
    nc = n ** 3
    rng = np.random.default_rng(7)
    J, S, diag = rng.random((nnu, nc)), rng.random((nnu, nc)), rng.random((nnu, nc))
    B = rng.random((nnu, nc)) if b_per_cell else rng.random(nnu)
    Bfull = B if b_per_cell else B[:, None]
    dev = lambda a: torch.as_tensor(a, device="cuda").contiguous()
    with rt.DiffuseTransfer() as e:
        e.set_uniform_grid(n, 1.0)
        Jd, Bd, Dd, Sd = dev(J), dev(B), dev(diag), dev(S)
        change, size = e.source_update_device(nnu, eps, Bd.data_ptr(), b_per_cell, Jd.data_ptr(), Dd.data_ptr(), Sd.data_ptr())
        want = numpy_update(S, J, Bfull, diag, eps)
        got = Sd.cpu().numpy()
        rel = np.abs(got - want).max() / np.abs(want).max()
        print(f"update kernel vs numpy: max rel {rel:.3e}, bitwise {np.array_equal(got, want)}")
        assert np.all(np.abs(got - want) <= 4 * EPS * np.abs(want))
        assert np.array_equal(got, want)  # IEEE operations in the stated order, nothing fused
        assert change == np.abs(got - S).max() and size == np.abs(got).max()
        # without the diagonal: the plain update, as the torch expressions of SourceIteration.step() give it
        Sd = dev(S)
        change, size = e.source_update_device(nnu, eps, Bd.data_ptr(), b_per_cell, Jd.data_ptr(), None, Sd.data_ptr())
        plain = torch.mul(Jd, 1.0 - eps)
        plain.add_(Bd if b_per_cell else Bd[:, None].expand(nnu, nc), alpha=eps)
        assert torch.equal(Sd, plain)
        assert change == float((plain - dev(S)).abs().max()) and size == float(plain.abs().max())
        # a denominator that is not positive: an error that names the element, S untouched
        bad = diag.copy()
        bad[1, 77] = 1.0 / (1.0 - eps) + 1e-3
        bad[2, 5] = 2.0
        Sd, Dd = dev(S), dev(bad)
        with pytest.raises(rt.FtteError) as err:
            e.source_update_device(nnu, eps, Bd.data_ptr(), b_per_cell, Jd.data_ptr(), Dd.data_ptr(), Sd.data_ptr())
        assert err.value.status == "FTTE_ERR_ARG" and f"element {nc + 77} " in str(err.value)
        assert np.array_equal(Sd.cpu().numpy(), S)


def errors_of(it, steps, Sc, eps, B):
    errs, measures = [], []
    for _ in range(steps):
        measures.append(it.step())
        S = it.S.cpu().numpy() if it.accelerate else (1.0 - eps) * it.J.cpu().numpy() + eps * B
        errs.append(np.abs(S - Sc).max() / np.abs(Sc).max())
    return np.array(errs), np.array(measures)


def test_same_fixed_point_fewer_iterations():
    """Plane-parallel tau_cell = 1e-2 ... 10 along storage-i, eps = 1e-2, B = 1, no inflow, 16^3, 48 directions.  On the host
    restatement: error of S against the converged solution after 50 iterations 0.31 (Lambda) / 0.029 (diagonal) / 8.0e-6
    (diagonal + Ng); iterations to an error below 1e-2: 184 / 65 / 20, below 1e-6: - / 185 / 56."""
    n, eps, Bv = 16, 1e-2, 1.0
    phi, theta, w = O.healpix_directions(2)
    tau = np.logspace(-2, 1, n)
    kappa = np.ascontiguousarray(np.broadcast_to((tau * n)[:, None, None], (n, n, n)).reshape(1, -1))
    uvb = np.zeros(1)
    shape = (1, n ** 3)
    diag = H.probe_uniform(n, kappa, 1.0, phi, theta, w)

    def sweep(S):
        return O.sweep_uniform(n, kappa, 1.0, phi, theta, w, uvb, src=S, arith=O.ARITH_DEVICE)
    Sc, m = H.iterate(sweep, "diagonal+ng", 150, eps, Bv, shape, diag)
    assert m[-1] < 1e-13
    host_err, host_measure, gpu_err, gpu_measure = {}, {}, {}, {}
    with rt.DiffuseTransfer() as e:
        e.set_uniform_grid(n, 1.0)
        e.set_opacity(kappa)
        for scheme in SCHEMES:
            errs = []
            _, host_measure[scheme] = H.iterate(sweep, scheme, 64, eps, Bv, shape, diag,
                                                on_step=lambda k, S: errs.append(np.abs(S - Sc).max() / np.abs(Sc).max()))
            host_err[scheme] = np.array(errs)
            it = SourceIteration(e, 1, n ** 3, phi, theta, w, uvb, eps, np.array([Bv]), accelerate=scheme)
            gpu_err[scheme], gpu_measure[scheme] = errors_of(it, 64, Sc, eps, Bv)
            print(scheme, "error after 10/25/50:", [f"{gpu_err[scheme][k - 1]:.3e}" for k in (10, 25, 50)],
                  "host:", [f"{host_err[scheme][k - 1]:.3e}" for k in (10, 25, 50)])
            # the same scheme, the same measure: the two differ by the rounding of sums only
            assert np.allclose(gpu_measure[scheme][:30], host_measure[scheme][:30], rtol=1e-6, atol=0), scheme
        assert gpu_err["diagonal+ng"][49] <= 1e-3 * gpu_err[None][49]
        assert gpu_err["diagonal"][49] <= 0.2 * gpu_err[None][49]
        host_count = int(np.argmax(host_err["diagonal+ng"] < 1e-6)) + 1
        assert host_err["diagonal+ng"][host_count - 1] < 1e-6
        reached = np.flatnonzero(gpu_err["diagonal+ng"] < 1e-6)
        assert len(reached) and reached[0] + 1 <= host_count + 4, (reached[:1], host_count)
        assert gpu_err[None][:host_count + 4].min() >= 1e-2  # the plain iteration is nowhere near by then
        # the fixed point did not move
        it = SourceIteration(e, 1, n ** 3, phi, theta, w, uvb, eps, np.array([Bv]), accelerate="diagonal+ng")
        it.run(150)
        end = np.abs(it.S.cpu().numpy() - Sc).max() / np.abs(Sc).max()
        print(f"150 Ng steps: {end:.3e} from the host's converged S; Ng reached 1e-6 after {reached[0] + 1} steps (host {host_count})")
        assert end <= 1e-10


def residual(e, it, eps, B, phi, theta, w, uvb):
    """max |(1 - eps) Lambda[S] + eps B - S| / max |S|, Lambda[S] by one plain sweep with S"""
    import torch
    S = it.S if it.accelerate else (1.0 - eps) * it.J + eps * it.B
    S = S.contiguous()
    torch.cuda.synchronize()
    e.set_source_function_device(S.data_ptr())
    J = torch.empty_like(S)
    e.transport_device(phi, theta, w, uvb, J.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    r = ((1.0 - eps) * J + eps * it.B - S).abs().max() / S.abs().max()
    return float(r)


def test_refined_block_converges_to_the_fixed_point():
    """64^3 with an optically thick 32^3 block refined once (hybrid sweep, fine bricks), eps = 0.1"""
    n, lo, eps, nnu = 64, (16, 16, 16), 0.1, 2
    blocks = [(lo[0] + a, lo[1] + b, lo[2] + c) for a in range(32) for b in range(32) for c in range(32)]
    level = synthetic.refine_levels(n, blocks, depth=1)
    rho = synthetic.lognormal_density(len(level), seed=9, sigma_ln=0.5)
    kappa = np.stack([(0.05 * n) * rho * np.where(level == 1, 40.0, 1.0) * f for f in (1.0, 0.3)])
    phi, theta, w = O.healpix_directions(2)
    uvb, B = np.zeros(nnu), np.array([1.0, 0.5])
    with rt.DiffuseTransfer() as e:
        e.set_grid(n, level, 1.0)
        e.set_opacity(kappa)
        its = {s: SourceIteration(e, nnu, len(level), phi, theta, w, uvb, eps, B, accelerate=s) for s in SCHEMES}
        r20 = {}
        for s in SCHEMES:
            its[s].run(20)
            r20[s] = residual(e, its[s], eps, B, phi, theta, w, uvb)
        assert e.counter("fine_block") == 64
        print("residual after 20 steps:", r20)
        assert r20["diagonal+ng"] < r20[None] and r20["diagonal"] < r20[None]
        its["diagonal+ng"].run(130)
        its["diagonal"].run(580)
        r_ng = residual(e, its["diagonal+ng"], eps, B, phi, theta, w, uvb)
        r_ali = residual(e, its["diagonal"], eps, B, phi, theta, w, uvb)
        print(f"residual after 150 Ng steps {r_ng:.3e}, after 600 diagonal steps {r_ali:.3e}")
        assert r_ng < 1e-10 and r_ali < 1e-10
        a, b = its["diagonal+ng"].S, its["diagonal"].S
        assert float((a - b).abs().max() / a.abs().max()) <= 1e-8


def test_without_accelerate_it_is_the_iteration_as_it_was(engine):
    import torch
    n, nnu, eps = 24, 2, 1e-2
    kappa, uvb, box = synthetic.uniform_workload(n, nnu, seed=3, tau_median=0.5)
    phi, theta, w = O.healpix_directions(1)
    Bv = np.array([1.0, 0.4])
    engine.set_uniform_grid(n, box)
    engine.set_opacity(kappa)
    it = SourceIteration(engine, nnu, n ** 3, phi, theta, w, uvb, eps, Bv)
    assert it.accelerate is None
    it.run(5)
    B = torch.as_tensor(Bv, device="cuda")[:, None].expand(nnu, n ** 3)
    J = torch.zeros((nnu, n ** 3), dtype=torch.float64, device="cuda")
    S = torch.empty_like(J)
    for _ in range(5):
        torch.mul(J, 1.0 - eps, out=S)
        S.add_(B, alpha=eps)
        torch.cuda.current_stream().synchronize()
        engine.set_source_function_device(S.data_ptr())
        engine.transport_device(phi, theta, w, uvb, J.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert torch.equal(it.J, J)
    engine.set_source_function(None)


def test_configs4_at_full_size():
    """BASELINE configs[4], 256^3 x 8 groups x 96 directions, eps = 1e-2: 12 steps of each scheme.  Only the order of the
    fixed-point residuals is asserted (a diagonal operator gains less the more cells the thick part has)."""
    import torch
    n, nnu, ndir, eps = 256, 8, 96, 1e-2
    _, s_nu, uvb = synthetic.frequency_groups(nnu)
    tau_cell = 10.0 ** (-2.0 + 3.0 * (np.arange(n) + 0.5) / n)
    kappa = np.ascontiguousarray(((tau_cell * n)[None, :, None, None] * s_nu[:, None, None, None] * np.ones((1, 1, n, n))).reshape(nnu, n ** 3))
    phi, theta, w = rt.healpix_directions(3, ndir)
    uvb, B = uvb * 0.0 + 1e-30, 1e-21 * s_nu ** 0.5
    r = {}
    with rt.DiffuseTransfer() as e:
        e.set_uniform_grid(n, 1.0)
        e.set_opacity(kappa)
        del kappa
        for s in SCHEMES:
            it = SourceIteration(e, nnu, n ** 3, phi, theta, w, uvb, eps, B, accelerate=s)
            it.run(12)
            assert bool(torch.isfinite(it.S).all()) and bool(torch.isfinite(it.J).all()) and float(it.S.min()) >= 0
            r[s] = residual(e, it, eps, B, phi, theta, w, uvb)
            del it
            torch.cuda.empty_cache()
    print("configs[4] at 256^3, residual after 12 steps:", {str(k): f"{v:.4e}" for k, v in r.items()})
    assert r["diagonal+ng"] < r[None] and r["diagonal"] < r[None]
