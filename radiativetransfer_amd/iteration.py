"""Source iteration on top of the sweep (BASELINE configs[4]: strong scattering, many iterations).

The reference's own iteration couples J to the opacities through its chemistry (solveRateEquations, out of scope
here); its transport has the emission term switched off.  For scattering problems the build defines the usual
two-level-atom source function

    S_nu = (1 - eps) J_nu + eps B_nu ,       Iout = Iin exp(-tau) + S (1 - exp(-tau))   (ftte_set_source_function)

and iterates  J^{k+1} = Lambda[S(J^k)]  (Lambda iteration): one sweep per iteration, J and S stay on the device.  Over several
ranks (`shard`: distributed.Shard2D, frequency groups first, then directions) a rank keeps J and S of ITS groups only -- the
source function of a group needs that group's J and nothing else --, so with as many ranks as groups nothing is exchanged at all,
and where the directions are split too one all-reduce of the rank's groups over its direction slices closes an iteration.
Fixed points: J = B wherever the medium is thick; J = inflow in radiative equilibrium with the boundary (tested).

A plain Lambda iteration changes little per step long before it is converged (with eps = 1e-2 the change goes like 1/k).  Two
accelerated schemes with the SAME fixed point (`accelerate=`):

    "diagonal"     approximate-operator (Jacobi) iteration with the exact diagonal of the discrete Lambda operator,
                       S <- S + ((1 - eps) J + eps B - S) / (1 - (1 - eps) Lambda*),
                   Lambda* from DiffuseTransfer.lambda_diagonal_device (a cell's own S enters its own J only through
                   S (1 - g(tau)) per segment: local, exact, one pass over the opacities), the update one kernel pass
    "diagonal+ng"  the same, plus Ng's extrapolation of S from the last four iterates, per frequency group, every
                   `ng_period` steps
"""
from __future__ import annotations

from typing import Optional

import numpy as np


class SourceIteration:
    def __init__(self, engine, nnu: int, ncell: int, phi, theta, weight, uvb, epsilon: float, planck, device="cuda:0",
                 group=None, shard=None, stage_on_host: bool = False, accelerate: Optional[str] = None, ng_start: int = 4,
                 ng_period: int = 4):
        """engine: a DiffuseTransfer with grid and opacities set; planck: B_nu, [nnu] or [nnu][ncell];
        phi/theta/weight: THIS rank's share of the direction list (weights of all ranks sum to the quadrature's total).
        group: all ranks sweep all groups for a share of the directions (one all-reduce of J per iteration over `group`).
        shard: a Shard2D -- nnu, uvb, planck and the engine's opacities are then those of THIS rank's groups (shard.groups), the
        directions its share (shard.directions); stage_on_host as in Shard2D.sum_directions.
        accelerate: None (the plain Lambda iteration), "diagonal" or "diagonal+ng" (module docstring).  Ng's extrapolation is
        made after a step once `ng_start` steps are done and then after every `ng_period`-th step (ng_period >= 4: the four
        iterates it uses are then all younger than the last extrapolation)."""
        import torch
        self.torch = torch
        self.engine = engine
        self.phi, self.theta, self.weight = (np.ascontiguousarray(a, dtype=np.float64) for a in (phi, theta, weight))
        self.uvb = np.ascontiguousarray(uvb, dtype=np.float64)
        self.eps = float(epsilon)
        self.group = group
        self.shard, self.stage_on_host = shard, stage_on_host
        dev = torch.device(device)
        B = torch.as_tensor(np.asarray(planck, dtype=np.float64), device=dev)
        self.B = B[:, None].expand(nnu, ncell) if B.dim() == 1 else B
        self.J = torch.zeros((nnu, ncell), dtype=torch.float64, device=dev)
        self.S = torch.empty_like(self.J)
        self.iterations = 0
        if accelerate not in (None, "diagonal", "diagonal+ng"):
            raise ValueError('accelerate must be None, "diagonal" or "diagonal+ng"')
        if accelerate == "diagonal+ng" and (ng_start < 4 or ng_period < 4):
            raise ValueError("Ng's extrapolation needs four iterates: ng_start >= 4 and ng_period >= 4")
        if accelerate is not None and group is not None:
            raise ValueError("accelerate: over several ranks use shard= (a Shard2D)")
        self.accelerate, self.ng_start, self.ng_period = accelerate, int(ng_start), int(ng_period)
        self.nnu = nnu
        self.diag = None          # Lambda*, made at the first accelerated step (refresh() makes it anew)
        self.lambda_ms = None     # device time of the last Lambda* call
        self.history = []         # the last iterates of S, oldest first (Ng)
        self.extrapolations = 0
        if accelerate is not None:
            self.B_dev = B.contiguous()
            self.b_per_cell = B.dim() == 2
            torch.mul(self.J, 1.0 - self.eps, out=self.S)  # the plain iteration's first source function: J = 0
            self.S.add_(self.B, alpha=self.eps)

    def refresh(self):
        """Lambda* anew: after new opacities, a new grid or another direction list (accelerated modes)."""
        if self.accelerate is None:
            return
        torch = self.torch
        if self.diag is None:
            self.diag = torch.empty_like(self.J)
        cur = torch.cuda.current_stream()
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record(cur)
        self.engine.lambda_diagonal_device(self.phi, self.theta, self.weight, self.diag.data_ptr(), cur.cuda_stream)
        t1.record(cur)
        cur.synchronize()
        self.lambda_ms = t0.elapsed_time(t1)
        if self.shard is not None:  # this rank's directions are a share: the diagonal is additive over the direction list
            self.shard.sum_directions(self.diag, self.stage_on_host)

    def _ng(self):
        """Ng's extrapolation (the three-term form: the 2 x 2 unweighted least-squares system from the differences of the last
        four iterates), group by group; a group whose system is singular keeps its iterate."""
        torch = self.torch
        y3, y2, y1, y0 = self.history  # y0 the newest
        for g in range(self.nnu):
            # a group at a time, as vectors: the sums do not depend on how many groups this rank holds
            q1 = y0[g] - 2.0 * y1[g] + y2[g]
            q2 = y0[g] - y1[g] - y2[g] + y3[g]
            q3 = y0[g] - y1[g]
            A1, B1, B2, C1, C2 = (float(v) for v in torch.stack([torch.dot(q1, q1), torch.dot(q1, q2), torch.dot(q2, q2),
                                                                  torch.dot(q1, q3), torch.dot(q2, q3)]).cpu())
            det = A1 * B2 - B1 * B1
            if not np.isfinite(det) or det == 0.0 or abs(det) <= 1e-30 * abs(A1 * B2):
                continue
            a, b = (C1 * B2 - C2 * B1) / det, (C2 * A1 - C1 * B1) / det
            self.S[g].copy_((1.0 - a - b) * y0[g] + a * y1[g] + b * y2[g])
        self.extrapolations += 1
        self.history = []

    def _step_accelerated(self) -> float:
        torch = self.torch
        if self.diag is None:
            self.refresh()
        cur = torch.cuda.current_stream()
        cur.synchronize()  # S is read by the library on the same stream; keep the hand-over simple
        self.engine.set_source_function_device(self.S.data_ptr())
        self.engine.transport_device(self.phi, self.theta, self.weight, self.uvb, self.J.data_ptr(), cur.cuda_stream)
        if self.shard is not None:
            self.shard.sum_directions(self.J, self.stage_on_host)
        change, size = self.engine.source_update_device(self.nnu, self.eps, self.B_dev.data_ptr(), self.b_per_cell, self.J.data_ptr(),
                                                        self.diag.data_ptr(), self.S.data_ptr(), cur.cuda_stream)
        self.iterations += 1
        if self.accelerate == "diagonal+ng":
            self.history.append(self.S.clone())
            if len(self.history) > 4:
                self.history.pop(0)
            k = self.iterations
            if k >= self.ng_start and (k - self.ng_start) % self.ng_period == 0 and len(self.history) == 4:
                self._ng()
        if self.shard is not None and self.shard.world > 1:  # the measure is over all groups: the largest of every rank's
            import torch.distributed as dist
            norms = torch.tensor([change, size], dtype=torch.float64, device="cpu" if self.stage_on_host else self.J.device)
            dist.all_reduce(norms, op=dist.ReduceOp.MAX)
            change, size = float(norms[0]), float(norms[1])
        return change / size if size > 0 else 0.0

    def step(self) -> float:
        """One iteration.  accelerate=None: returns max |J_new - J_old| / max |J_new| (the convergence measure of SURVEY.md
        section 8(d)).  Accelerated modes: returns max |S_new - S_old| / max |S_new| of the operator update (before an
        extrapolation), which the update kernel delivers for nothing.  Neither is an error estimate: a plain iteration with
        eps = 1e-2 changes by 1e-2 per step while it is still 30 % away from its fixed point."""
        if self.accelerate is not None:
            return self._step_accelerated()
        torch = self.torch
        torch.mul(self.J, 1.0 - self.eps, out=self.S)
        self.S.add_(self.B, alpha=self.eps)
        J_old = self.J.clone()
        stream = torch.cuda.current_stream().cuda_stream
        torch.cuda.current_stream().synchronize()  # S is read by the library on the same stream; keep the hand-over simple
        self.engine.set_source_function_device(self.S.data_ptr())
        self.engine.transport_device(self.phi, self.theta, self.weight, self.uvb, self.J.data_ptr(), stream)
        if self.shard is not None:
            self.shard.sum_directions(self.J, self.stage_on_host)
        else:
            from .distributed import allreduce_J
            allreduce_J(self.J, self.group)
        self.iterations += 1
        norms = torch.stack([(self.J - J_old).abs().max(), self.J.abs().max()])
        if self.shard is not None and self.shard.world > 1:  # the measure is over all groups: the largest of every rank's
            import torch.distributed as dist
            if self.stage_on_host:
                norms = norms.cpu()
            dist.all_reduce(norms, op=dist.ReduceOp.MAX)
        return float(norms[0] / norms[1])

    def run(self, iterations: int, tol: Optional[float] = None):
        history = []
        for _ in range(iterations):
            history.append(self.step())
            if tol is not None and history[-1] < tol:
                break
        return history
