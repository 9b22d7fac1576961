"""Training loop pieces around the HIP RHS/VJP.

    Adam        — Flux 0.14 legacy `Adam(η, β=(0.9,0.999), ϵ=1e-8)` + `update!`
                  (LV_driver_KANODE.jl:219,287; Fisher-KPP_Source.jl:167,201;
                  Flux pinned at Lotka-Volterra/Manifest.toml:841): the torch statement
    FusedAdam   — the same step as ONE HIP launch (kanode_adam_step) with the post-all-reduce
                  mean folded in; what Trainer uses on the GPU
    mse_loss    — `mean(abs2, X .- pred)` (LV_driver_KANODE.jl:197-203, Fisher-KPP_Source.jl:107-109)
    reg_loss    — L1 + entropy on the flat p (LV_driver_KANODE.jl:187-194)
    EnsembleTrainer — R independent Trainers of one problem; on the GPU all of them in one launch per chunk
    Trainer     — one iteration = forward Tsit5 solve, loss, the gradient by the
                  InterpolatingAdjoint (the reference's NeuralODE default sensealg; native
                  kanode_adjoint_tsit5 on the GPU) wherever the RHS provides the adjoint stage,
                  ForwardDiffSensitivity for a small hand-written ODEProblem (the Fisher-KPP /
                  Allen-Cahn source drivers at their own sizes: SciMLSensitivity's automatic
                  choice; native kanode_forward_sensitivity_tsit5),
                  else the discrete adjoint (reverse mode through the stages), ONE all-reduce
                  of [∂L/∂p ; L] across the trajectory shards (RCCL over xGMI with backend
                  "nccl"; gloo on CPU), then the identical Adam step on every rank.
"""
from __future__ import annotations

import torch

from .adjoint import forward_ok, native_forward_dense, native_mse_gradient, native_mse_gradient_forward
from .ode import Solution, Tsit5Options, _saveat_list, native_ok, solve, solve_ensemble


class Adam:
    """Flux.Optimise.Adam (legacy API):  mt = β1 mt + (1-β1) Δ;  vt = β2 vt + (1-β2) Δ²;
    Δ = mt / (1-β1^t) / (√(vt / (1-β2^t)) + ϵ) · η;  x .-= Δ.

    Flux evaluates these broadcasts with its Float64 hyper-parameters, so Float32 x, mt, vt are
    promoted, computed in Float64 and rounded on store; apply! stores the step into the gradient array
    (Float32 with Float32 parameters) and update! subtracts it in Float32.  This torch statement does the same, in the
    operation order of the fused kernel (kan_optim.hip: every product and sum rounded separately), so
    the CPU and GPU trainers take the same optimiser trajectory for either dtype."""

    def __init__(self, eta: float = 1e-3, beta=(0.9, 0.999), eps: float = 1e-8):
        self.eta, self.beta, self.eps = eta, beta, eps
        self.state = {}

    def apply(self, x: torch.Tensor, d: torch.Tensor) -> torch.Tensor:
        """Advances the moments; returns the Float64 step Δ (x is not changed)."""
        b1, b2 = self.beta
        st = self.state.get(id(x))
        if st is None:
            st = [torch.zeros_like(x), torch.zeros_like(x), [b1, b2]]
            self.state[id(x)] = st
        mt, vt, bp = st
        d64 = d.double()
        m64 = b1 * mt.double() + (1.0 - b1) * d64
        v64 = b2 * vt.double() + ((1.0 - b2) * d64) * d64
        mt.copy_(m64)                                   # the stored moments (rounded for Float32)
        vt.copy_(v64)
        den = torch.sqrt(vt.double() / (1.0 - bp[1])) + self.eps
        step = (mt.double() / (1.0 - bp[0])) / den * self.eta
        bp[0] *= b1
        bp[1] *= b2
        return step

    def update(self, x: torch.Tensor, d: torch.Tensor) -> None:
        """Flux.update!(opt, x, Δ): x .-= apply!(opt, x, Δ), the step rounded to x's dtype (apply! stores it
        into the gradient array) and subtracted in that dtype."""
        with torch.no_grad():
            x.sub_(self.apply(x, d).to(x.dtype))


class FusedAdam(Adam):
    """Adam whose step is one kanode_adam_step launch on x's device (m, v device-resident, Flux's
    running powers βp kept on the host).  update(x, g, scale) applies Δ = scale·g: Trainer passes the
    SUM all-reduced gradient with scale = 1/world_size, so the mean, both moments and x -= Δ are one
    pass over the parameters instead of ~8 torch launches."""

    def update(self, x: torch.Tensor, d: torch.Tensor, scale: float = 1.0) -> None:
        from . import _lib as L
        if not x.is_cuda:
            raise L.KanodeError("FusedAdam runs on the GPU (kanode_adam_step); use kanode.Adam on the CPU")
        if x.dtype not in (torch.float32, torch.float64) or d.dtype != x.dtype or d.numel() < x.numel():
            raise L.KanodeError("FusedAdam: x and the gradient must share a float dtype and size")
        if not (x.is_contiguous() and d.is_contiguous()):
            raise L.KanodeError("FusedAdam: x and the gradient must be contiguous")
        b1, b2 = self.beta
        st = self.state.get(id(x))
        if st is None:
            st = [torch.zeros_like(x), torch.zeros_like(x), [b1, b2]]
            self.state[id(x)] = st
        mt, vt, bp = st
        dt = L.F64 if x.dtype == torch.float64 else L.F32
        stream = torch.cuda.current_stream(x.device).cuda_stream
        L.check(L.lib().kanode_adam_step(x.data_ptr(), mt.data_ptr(), vt.data_ptr(), d.data_ptr(), x.numel(), dt,
                                         float(scale), float(self.eta), float(b1), float(b2), float(self.eps),
                                         float(bp[0]), float(bp[1]), stream), None, "kanode_adam_step")
        bp[0] *= b1
        bp[1] *= b2


def mse_loss(pred: torch.Tensor, target: torch.Tensor) -> torch.Tensor:
    """mean((target - pred)²) (the drivers' loss, Fisher-KPP_Source.jl:107-108 mean(abs2, X - pred)): torch's
    fused mse_loss, one launch forward and one backward instead of a sub / pow / mean chain."""
    return torch.nn.functional.mse_loss(pred, target)


def reg_loss(p: torch.Tensor, act_reg: float = 1.0, entropy_reg: float = 1.0) -> torch.Tensor:
    l1 = torch.abs(p)
    a = torch.sum(l1)
    e = l1 / a
    return a * act_reg + (-torch.sum(e * torch.log(e))) * entropy_reg


def _group_ranks(group) -> set[int]:
    import torch.distributed as dist
    if group is None or group is dist.group.WORLD:
        return set(range(dist.get_world_size()))
    return set(dist.get_process_group_ranks(group))


def _check_orthogonal(dp_group, tp_group) -> None:
    """The data-parallel gradient group of a grid-sharded trainer may share only this rank with the
    grid-shard group: every other member of dp_group must own the same parameter slice."""
    import torch.distributed as dist
    if tp_group is None or not dist.is_initialized():
        return
    shared = (_group_ranks(dp_group) & _group_ranks(tp_group)) - {dist.get_rank()}
    if dp_group is tp_group or shared:
        raise ValueError("Trainer(tp=True): `group` must be the data-parallel group orthogonal to the rhs's "
                         f"grid-shard group (it shares ranks {sorted(shared)}); all-reducing over it would add "
                         "gradients of different parameter slices")


class Trainer:
    """KAN-ODE training on a shard of trajectories.

    rhs(u, p, t) -> du must be differentiable (kanode.ChainRHS / FisherKPPRHS are:
    their backward is the HIP VJP).  `target` has the layout of the saved solution
    (len(saveat), *u0.shape).  `group` is a torch.distributed process group (or None)."""

    def __init__(self, rhs, u0, tspan, saveat, target, p0, eta: float = 5e-4, solver: Tsit5Options | None = None,
                 sparse_reg: float = 0.0, group=None, sensealg: str | None = None, tp: bool = False,
                 device_loop: str = "default"):
        """device_loop: which shapes run() keeps on the device.  "default": one Lotka-Volterra trajectory (and the
        Fisher-KPP forward loop).  "any": also every other small fp64 chain whose forward solve and adjoint each run
        in one workgroup (a pruned [2,k,2], a [3,6,3] chain, three layers, up to 16 trajectories): run() turns the
        handle's `train_any_chain` option on where it is off.  Its losses are summed on one wave, so they agree with
        step()'s torch-summed ones to rounding, not bitwise, which is why it is not the default.

        tp=True: `rhs` is grid-sharded (kanode.tp.GridShardedChainRHS); u0/target/p0 are this rank's
        slices, the loss is this shard's part of the global mean, gradients are shard-local.  `group`
        is then the ORTHOGONAL data-parallel group (ranks holding the same parameter slice for other
        trajectories); passing the grid-shard group would sum slices of different parameters, so a
        group sharing any rank with rhs.group other than this one is rejected."""
        if device_loop not in ("default", "any"):
            raise ValueError(f"Trainer: device_loop must be 'default' or 'any', not {device_loop!r}")
        self.device_loop = device_loop
        if tp and group is not None:
            _check_orthogonal(group, getattr(rhs, "group", None))
        self.rhs, self.u0, self.tspan, self.saveat, self.target = rhs, u0, tspan, saveat, target
        self.tp = tp
        self.p = p0.detach().clone()
        self.opt = FusedAdam(eta) if self.p.is_cuda else Adam(eta)
        self.solver = solver or Tsit5Options()
        self.sparse_reg = sparse_reg
        self.group = group
        self.history = []
        # the reference's default: NeuralODE passes InterpolatingAdjoint(autojacvec = ZygoteVJP()); a hand-written
        # ODEProblem (rhs.auto_sensealg: Fisher-KPP / Allen-Cahn source) gets SciMLSensitivity's automatic choice,
        # ForwardDiffSensitivity where length(u0) + length(p) <= 100 (resolved per step: "auto"); reverse mode
        # through the solver steps for an RHS without an adjoint stage
        if sensealg is None:
            sensealg = ("auto" if getattr(rhs, "auto_sensealg", False) else "interpolating_adjoint") \
                if hasattr(rhs, "vjp_stage") else "discrete"
        self.sensealg = sensealg
        self.last_run = None  # the loop the last run() took: "device_forward", "device_adjoint" or "host"
        self._pver = 0        # bumped by every optimiser update (keys the cached forward of eval_loss)
        self._pre = None      # (pver, path, forward payload) from eval_loss, consumed by the next step

    def predict(self, p) -> Solution:
        return solve(self.rhs, self.u0, self.tspan, p, self.saveat, self.solver, sensealg=self.sensealg)

    def _fast_path(self):
        """(saveat list, path) with path "forward" / "interpolating_adjoint" for the native plain-MSE step, or None.
        (sparse_reg does not exclude it: loss_and_grad adds the L1 term to the native loss and gradient.)"""
        sv = _saveat_list(self.tspan, self.saveat)
        tf = float(self.tspan[1])
        sv = [s for s in sv if s <= tf + 1e-12 * max(1.0, abs(tf))]     # as solve() filters them
        sa = self.sensealg
        fast = (not self.tp and tuple(self.target.shape) == (len(sv),) + tuple(self.u0.shape)
                and native_ok(self.rhs, self.u0, self.tspan, self.p, sv, self.solver))
        if sa == "auto":
            sa = "forward" if fast and forward_ok(self.rhs, self.u0, self.p) else "interpolating_adjoint"
        return sv, (sa if fast and sa in ("forward", "interpolating_adjoint") else None)

    def _drop_pre(self):
        if self._pre is not None and self._pre[1] == "interpolating_adjoint":
            self.rhs.hd.release_dense(self._pre[2][2])
        self._pre = None

    def eval_loss(self) -> float:
        """loss(p) at the current parameters, as the drivers log it after update! (LV_driver_KANODE.jl:289-290
        loss_train(p); Fisher-KPP_Source.jl:204).  On the native plain-MSE path this forward solve is exactly the
        next iteration's InterpolatingAdjoint forward (same p, u0, tspan, saveat), so its dense output is kept and
        the next step() takes its gradient from it instead of solving again.  The cache is keyed
        on the Trainer's own updates: change self.p only through step() (or call eval_loss again)."""
        self._drop_pre()
        sv, path = self._fast_path()
        if path == "interpolating_adjoint":
            pre = native_forward_dense(self.rhs, self.u0, self.tspan, self.p, sv, self.solver)
        else:
            # (in forward mode the next gradient is a Dual solve, whose error norm counts the partials: its steps
            # and values are not the logged plain solve's, so nothing is kept)
            with torch.no_grad():
                return float(mse_loss(solve(self.rhs, self.u0, self.tspan, self.p.detach(), self.saveat,
                                            self.solver).u, self.target))
        self._pre = (self._pver, path, pre)
        return float(mse_loss(pre[0], self.target))

    def loss_and_grad(self):
        sv, path = self._fast_path()
        pre = None
        if self._pre is not None:
            if self._pre[0] == self._pver and self._pre[1] == path:
                pre = self._pre[2]
                self._pre = None
            else:
                self._drop_pre()
        if path == "forward":
            # ForwardDiffSensitivity: one native call carrying ∂u/∂p (adjoint.native_mse_gradient_forward)
            loss, g, sol = native_mse_gradient_forward(self.rhs, self.u0, self.tspan, self.p, sv, self.solver,
                                                       self.target, pre=pre)
            return self._with_l1(loss.detach(), g) + (sol,)
        if path == "interpolating_adjoint":
            # the plain-MSE step through the two native calls directly (adjoint.native_mse_gradient)
            loss, g, sol = native_mse_gradient(self.rhs, self.u0, self.tspan, self.p, sv, self.solver, self.target,
                                               pre=pre)
            return self._with_l1(loss.detach(), g) + (sol,)
        p = self.p.detach().requires_grad_(True)
        sol = self.predict(p)
        if self.tp:   # Σ over the grid shards of these partial sums = the global mean
            loss = torch.sum((self.target - sol.u) ** 2) / self.rhs.global_count(sol.u.numel())
        else:
            loss = mse_loss(sol.u, self.target)
        if self.sparse_reg:
            loss = loss + reg_loss(p, self.sparse_reg, 0.0)
        (g,) = torch.autograd.grad(loss, p)
        return loss.detach(), g.detach(), sol

    def _with_l1(self, loss, g):
        """The native plain-MSE (loss, gradient) with the sparsity term of the driver's sparse_on = 1 added
        (LV_driver_KANODE.jl:187-201): loss + reg_loss(p, λ, 0) and g + λ·sign(p), formed on p's device before any
        all-reduce.  An entry of p that is exactly zero makes the loss NaN, as reg_loss is there."""
        if not self.sparse_reg:
            return loss, g
        p = self.p.detach()
        return loss + reg_loss(p, self.sparse_reg, 0.0), g + self.sparse_reg * torch.sign(p).reshape(g.shape)

    def step(self) -> float:
        return self._step()[0]

    def _step(self):
        """One iteration: (loss, this rank's gradient, the forward Solution)."""
        loss, g, sol = self.loss_and_grad()
        g_own = g
        if self.tp:
            loss = torch.as_tensor(self.rhs.reduce_sum(float(loss)), dtype=g.dtype)
        scale = 1.0
        if self.group is not None:
            import torch.distributed as dist
            ws = dist.get_world_size(self.group)
            buf = torch.cat([g.reshape(-1), loss.reshape(1).to(device=g.device, dtype=g.dtype)])   # one collective per step
            dist.all_reduce(buf, op=dist.ReduceOp.SUM, group=self.group)
            scale = 1.0 / ws
            g, loss = buf[:-1].reshape(g.shape), buf[-1] * scale
        if isinstance(self.opt, FusedAdam):
            self.opt.update(self.p, g.contiguous(), scale)      # the mean is formed inside the launch
        else:
            self.opt.update(self.p, g * scale if scale != 1.0 else g)
        self._pver += 1
        lv = float(loss)
        self.history.append(lv)
        return lv, g_own, sol

    def _native_run_path(self, with_test: bool = False):
        """The device-resident loop run() takes, or None: "device_adjoint" (kanode_train_tsit5: the MSE, plus the L1
        term with sparse_reg, on the InterpolatingAdjoint) or "device_forward" (kanode_train_forward_tsit5: the
        plain-MSE forward-mode gradient of a small Fisher-KPP field, never with sparse_reg; with_test: with its
        logged-loss solve), where the handle covers the shape, the
        gradient is this rank's alone and the optimiser is FusedAdam."""
        hd = getattr(self.rhs, "hd", None)
        if (hd is None or self.sensealg not in ("interpolating_adjoint", "forward", "auto") or self.group is not None
                or self.tp or type(self.opt) is not FusedAdam or not self.p.is_cuda):
            return None
        if self.p.dtype != torch.float64 or not (self.p.is_contiguous() and self.u0.is_contiguous()):
            return None
        if self.solver.control != "auto" or self.solver.replay_dts is not None \
                or self.solver.replay_adjoint_dts is not None:
            return None                                   # (host / hipGraph step control, replayed steps: step())
        B = self.u0.shape[0] if self.u0.dim() == 2 else 1
        path = self._fast_path()[1]                       # ("auto" resolved; it turns fsens_wide on where it applies)
        if path == "interpolating_adjoint" and self.sensealg == "interpolating_adjoint":
            if self.device_loop == "any" and hd.get_option("train_any_chain") == 0:
                hd.set_option("train_any_chain", 1)       # (idempotent, as "auto" turns fsens_wide on)
            if hd.train_supported(B):
                return "device_adjoint"
        if path == "forward" and not self.sparse_reg and hd.train_forward_supported(B, with_test):
            return "device_forward"                       # (no L1 term in the Fisher-KPP loop: step() serves it)
        return None

    def run(self, n_iters: int, test=None, chunk: int = 256, record: bool = False) -> dict:
        """n_iters iterations of the driver loop (LV_driver_KANODE.jl:279-291): step(), and with
        test = (tspan_test, saveat_test, target_test) the test loss at the updated parameters after each.
        Returns {"loss": [n_iters] (loss[it] at p_it, before the update, as step() returns it), "loss_test":
        [n_iters] or None (loss_test[it] at p_{it+1})}, float64 CPU tensors; with record=True also "grad",
        "p_before" ([n_iters, P], on p's device) and "counts" ([n_iters, 4] int64, CPU: forward naccept, nreject,
        adjoint naccept, nreject).

        Where the handle covers it (one Lotka-Volterra trajectory on the InterpolatingAdjoint; with
        Trainer(device_loop="any") every small chain of the one-workgroup solve and adjoint, at up to 16 trajectories;
        or a small Fisher-KPP field on the forward-mode gradient -- explicitly or through "auto" --; fp64, FusedAdam,
        no group; sparse_reg adds the L1 term inside the InterpolatingAdjoint loops and sends a Fisher-KPP field to the
        host loop)
        the iterations run on the device (self.last_run says which loop ran: "device_adjoint", "device_forward" or
        "host"; on the forward loop there is no adjoint, and counts[:, 2:] are the logged-loss solve's naccept and nreject
        when a test problem is given, else zero), at most `chunk` per kernel launch (no single kernel runs for long on a shared
        machine): the optimiser's own m, v and running powers are used and advanced.  If the device loop stops (a
        solve at maxiters, the dense-output capacity, a non-finite loss) the iterations before it are kept in
        history and a KanodeError names the iteration and reason, p, m, v as the last good iteration left them.
        Everything else is a plain loop of step() plus the test solve, on the CPU too.  The cached forward of
        eval_loss is dropped either way."""
        n_iters = int(n_iters)
        if n_iters < 0 or chunk < 1:
            raise ValueError("run: n_iters >= 0 and chunk >= 1")
        if test is not None:
            tspan_t, saveat_t, target_t = test
            sv_t = _saveat_list(tspan_t, saveat_t)
            sv_t = [s for s in sv_t if s <= float(tspan_t[1]) + 1e-12 * max(1.0, abs(float(tspan_t[1])))]
        dev = self._native_run_path(test is not None) if n_iters > 0 else None
        if dev is not None and (test is None or (float(tspan_t[0]) == float(self.tspan[0])
                                                 and tuple(target_t.shape) == (len(sv_t),) + tuple(self.u0.shape))):
            self.last_run = dev
            return self._run_native(n_iters, None if test is None else (float(tspan_t[1]), sv_t, target_t),
                                    int(chunk), record, forward=dev == "device_forward")
        self.last_run = "host"
        loss, loss_t, grads, pbs, counts = [], [], [], [], []
        for _ in range(n_iters):
            if record:
                pbs.append(self.p.detach().clone())
            lv, g, sol = self._step()
            loss.append(lv)
            if record:
                grads.append(g.detach().clone().reshape(-1))
                adj = sol.stats.get("adjoint", {})
                counts.append([sol.stats.get("naccept", 0), sol.stats.get("nreject", 0), adj.get("naccept", 0),
                               adj.get("nreject", 0)])
            if test is not None:
                with torch.no_grad():
                    loss_t.append(float(mse_loss(solve(self.rhs, self.u0, tspan_t, self.p.detach(), saveat_t,
                                                       self.solver).u, target_t)))
        self._drop_pre()
        out = {"loss": torch.tensor(loss, dtype=torch.float64),
               "loss_test": torch.tensor(loss_t, dtype=torch.float64) if test is not None else None}
        if record:
            P = self.p.numel()
            out["grad"] = torch.stack(grads) if grads else self.p.new_zeros((0, P))
            out["p_before"] = torch.stack(pbs).reshape(len(pbs), P) if pbs else self.p.new_zeros((0, P))
            out["counts"] = torch.tensor(counts, dtype=torch.int64).reshape(len(counts), 4)
        return out

    def _run_native(self, n_iters: int, test, chunk: int, record: bool, forward: bool = False) -> dict:
        from . import _lib as L
        hd = self.rhs.hd
        self._drop_pre()
        sv, _ = self._fast_path()
        b1, b2 = self.opt.beta
        st = self.opt.state.get(id(self.p))
        if st is None:                                    # as FusedAdam.update creates them
            st = [torch.zeros_like(self.p), torch.zeros_like(self.p), [b1, b2]]
            self.opt.state[id(self.p)] = st
        mt, vt, bp = st
        oc = self.solver.to_c()
        target = self.target.contiguous()
        if test is not None:
            test = (test[0], test[1], test[2].contiguous())
        parts, left, err = [], n_iters, None
        while left > 0 and err is None:
            k = min(left, chunk)
            call, kw = (hd.train_forward_tsit5, {}) if forward else (hd.train_tsit5, {"l1": float(self.sparse_reg)})
            r = call(self.p, mt, vt, self.u0, float(self.tspan[0]), float(self.tspan[1]), sv, target, oc,
                     self.opt.eta, (b1, b2), self.opt.eps, bp, k, test=test, record=record, **kw)
            d = r["iters_done"]
            for _ in range(d):                            # Flux's βp .*= β, once per iteration done
                bp[0] *= b1
                bp[1] *= b2
            self._pver += d
            self.history.extend(r["loss"][:d].tolist())
            parts.append((r, d))
            left -= k
            if r["error"] is not None:
                err = (n_iters - left - k + d, r["stop"], r["error"])
        self._drop_pre()
        if err is not None:
            raise L.KanodeError(f"Trainer.run: stopped at iteration {err[0]} ({err[1]}): {err[2]}; "
                                f"p, m, v are those after {err[0]} iterations")

        def cat(key, cpu):
            t = torch.cat([r[key][:d] for r, d in parts])
            return t.cpu() if cpu else t
        out = {"loss": cat("loss", True), "loss_test": cat("loss_test", True) if test is not None else None}
        if record:
            out["grad"], out["p_before"], out["counts"] = cat("grad", False), cat("p_before", False), cat("counts", True)
        return out


class EnsembleTrainer:
    """R independent trainings of one problem side by side: seeds, learning rates or penalty weights.

    p0 is [R, P]; eta and sparse_reg are a float or a sequence of R.  Where the handle covers the problem (the
    conditions of Trainer.run's device loops, evaluated once for the shared problem) run() takes all live replicas
    through ONE launch per chunk, one workgroup each (kanode_train_ensemble_tsit5 /
    kanode_train_forward_ensemble_tsit5), and replica r computes bit for bit what Trainer computes from the same
    state.  Everything else is the host path: R Trainers stepped in turn, on the CPU too.

    State: p, m, v ([R, P]; row r is replica r's, and its Trainer's optimiser works on these rows in place), bp (R
    pairs of running powers), history (R lists), stopped ({r: (iterations the replica had done, reason)})."""

    def __init__(self, rhs, u0, tspan, saveat, target, p0, eta=5e-4, solver: Tsit5Options | None = None,
                 sparse_reg=0.0, sensealg: str | None = None, device_loop: str = "default"):
        """device_loop: Trainer's keyword, for every member.  "default": the device path is one Lotka-Volterra
        trajectory (and the Fisher-KPP forward loop).  "any": also every other small fp64 chain of
        Trainer(device_loop="any"), through kanode_fit_ensemble_tsit5; the Lotka-Volterra shape keeps its own entry
        and its bits."""
        if device_loop not in ("default", "any"):
            raise ValueError(f"EnsembleTrainer: device_loop must be 'default' or 'any', not {device_loop!r}")
        self.device_loop = device_loop
        if not isinstance(p0, torch.Tensor) or p0.dim() != 2 or p0.shape[0] < 1:
            raise ValueError("EnsembleTrainer: p0 must be a tensor of shape [R, P]")
        R = int(p0.shape[0])

        def per_replica(x, name):
            xs = [float(x)] * R if isinstance(x, (int, float)) else [float(e) for e in x]
            if len(xs) != R:
                raise ValueError(f"EnsembleTrainer: {name} must be a float or a sequence of R = {R} floats")
            return xs
        self.R = R
        self.eta, self.sparse_reg = per_replica(eta, "eta"), per_replica(sparse_reg, "sparse_reg")
        self.rhs, self.u0, self.tspan, self.saveat, self.target = rhs, u0, tspan, saveat, target
        self.solver = solver or Tsit5Options()
        self.p = p0.detach().clone().contiguous()
        self.m, self.v = torch.zeros_like(self.p), torch.zeros_like(self.p)
        self._members = []
        for r in range(R):        # replica r's Trainer works on row r of p, m, v in place
            tr = Trainer(rhs, u0, tspan, saveat, target, self.p[r], eta=self.eta[r], solver=self.solver,
                         sparse_reg=self.sparse_reg[r], sensealg=sensealg, device_loop=device_loop)
            tr.p = self.p[r]
            tr.opt.state[id(tr.p)] = [self.m[r], self.v[r], list(tr.opt.beta)]
            self._members.append(tr)
        self.sensealg = self._members[0].sensealg
        self.stopped = {}
        self.last_run = None      # "device_adjoint", "device_forward" or "host"
        self.last_predict = None  # the path of the last predict() / eval_loss(): "device" or "host"

    @property
    def bp(self):
        return [tr.opt.state[id(tr.p)][2] for tr in self._members]

    @property
    def history(self):
        return [tr.history for tr in self._members]

    def live(self):
        return [r for r in range(self.R) if r not in self.stopped]

    def member(self, r: int) -> Trainer:
        """A Trainer on clones of replica r's p, m, v, running powers and history: to continue one member alone,
        prune it or checkpoint it.  The ensemble is not changed by what happens to it."""
        src = self._members[r]
        tr = Trainer(self.rhs, self.u0, self.tspan, self.saveat, self.target, self.p[r], eta=self.eta[r],
                     solver=self.solver, sparse_reg=self.sparse_reg[r], sensealg=src.sensealg,
                     device_loop=self.device_loop)
        tr.opt.state[id(tr.p)] = [self.m[r].clone(), self.v[r].clone(), list(self.bp[r])]
        tr.history = list(src.history)
        tr._pver = src._pver
        return tr

    def best(self):
        """(r, loss): the live replica with the smallest last recorded loss."""
        cand = [(tr.history[-1], r) for r, tr in enumerate(self._members) if r not in self.stopped and tr.history]
        if not cand:
            raise ValueError("EnsembleTrainer.best: no live replica has a recorded loss")
        loss, r = min(cand)
        return r, loss

    def predict(self, tspan=None, saveat=None):
        """The trajectories of all R replicas at their current parameters (kanode.solve_ensemble: one launch where
        the handle covers the problem), over the training span and saveat or the given ones, stopped replicas
        included.  Returns an EnsembleSolution; last_predict records its path ("device" / "host").  Touches neither
        p, m, v, the histories nor the members' cached forward."""
        sol = solve_ensemble(self.rhs, self.u0, self.tspan if tspan is None else tspan, self.p,
                             self.saveat if tspan is None and saveat is None else saveat, self.solver)
        self.last_predict = sol.path
        return sol

    def eval_loss(self, test=None) -> list:
        """mse_loss(u[r], target) of every replica at its current parameters, as R floats (NaN for a replica whose
        solve reached maxiters): against the training target, or a held-out (tspan, saveat, target) triple."""
        tspan, saveat, target = (None, None, self.target) if test is None else test
        sol = self.predict(tspan, saveat)
        return [float(mse_loss(sol.u[r], target)) for r in range(self.R)]

    def default_chunk(self, n_live: int) -> int:
        """The largest chunk with ceil(n_live / CUs) * chunk <= 256 (at least 1): workgroups beyond one per compute
        unit run in waves, and one launch stays as long as Trainer.run's 256-iteration launch."""
        if not self.p.is_cuda:
            return 256
        cus = torch.cuda.get_device_properties(self.p.device).multi_processor_count
        return max(1, 256 // -(-n_live // max(1, cus)))

    def _device_path(self, with_test: bool):
        probe = next((tr for tr in self._members if tr.sparse_reg), self._members[0])
        hd = getattr(self.rhs, "hd", None)
        if self.device_loop == "any":                     # (the members turn the option on, as Trainer.run does)
            return probe._native_run_path(with_test)
        if hd is not None and self.p.is_cuda and hd.get_option("train_any_chain"):
            with hd.options(train_any_chain=0):           # (the default's ensemble entry is the Lotka-Volterra shape's)
                return probe._native_run_path(with_test)
        return probe._native_run_path(with_test)          # (a penalty on any replica sends a Fisher-KPP field to the host)

    def run(self, n_iters: int, test=None, chunk: int | None = None, record: bool = False) -> dict:
        """n_iters iterations of every live replica.  Returns Trainer.run's dict with a leading replica dimension
        (loss, loss_test [R, n_iters]; with record grad, p_before [R, n_iters, P] and counts [R, n_iters, 4]) plus
        iters_done (R ints, this run's) and stop (R reason names, "ok" for a replica that ran through).

        A replica that stops (a solve at maxiters, the dense-output capacity, a non-finite loss) does not raise:
        it keeps the p, m, v of its last good iteration, its later entries of loss are NaN (its records zero), it
        enters self.stopped and later runs leave it out.  run raises only when every replica has stopped."""
        from . import _lib as L
        n_iters = int(n_iters)
        if n_iters < 0 or (chunk is not None and chunk < 1):
            raise ValueError("run: n_iters >= 0 and chunk >= 1")
        if not self.live():
            raise L.KanodeError(f"EnsembleTrainer.run: every replica has stopped: {self.stopped}")
        R, P = self.R, self.p.shape[1]
        nan = float("nan")
        out = {"loss": torch.full((R, n_iters), nan, dtype=torch.float64),
               "loss_test": torch.full((R, n_iters), nan, dtype=torch.float64) if test is not None else None}
        if record:
            out["grad"], out["p_before"] = self.p.new_zeros((R, n_iters, P)), self.p.new_zeros((R, n_iters, P))
            out["counts"] = torch.zeros((R, n_iters, 4), dtype=torch.int64)
        done, stop = [0] * R, ["ok"] * R
        dev, tst = None, None
        if test is not None:
            tspan_t, saveat_t, target_t = test
            sv_t = _saveat_list(tspan_t, saveat_t)
            sv_t = [s for s in sv_t if s <= float(tspan_t[1]) + 1e-12 * max(1.0, abs(float(tspan_t[1])))]
        if n_iters > 0:
            dev = self._device_path(test is not None)
            if dev is not None and test is not None:
                if float(tspan_t[0]) == float(self.tspan[0]) and tuple(target_t.shape) == (len(sv_t),) + tuple(self.u0.shape):
                    tst = (float(tspan_t[1]), sv_t, target_t.contiguous())
                else:
                    dev = None
        self.last_run = dev or "host"
        if dev is None:
            self._run_host(n_iters, test, record, out, done, stop)
        else:
            self._run_native(n_iters, tst, chunk, record, dev == "device_forward", out, done, stop)
        out["iters_done"], out["stop"] = done, stop
        if not self.live():
            raise L.KanodeError(f"EnsembleTrainer.run: every replica has stopped: {self.stopped}")
        return out

    def _stop(self, r, reason, stop):
        self.stopped[r] = (len(self._members[r].history), reason)
        stop[r] = reason

    def _run_host(self, n_iters, test, record, out, done, stop):
        import math
        for r in self.live():
            tr = self._members[r]
            for it in range(n_iters):
                st = tr.opt.state[id(tr.p)]
                keep = (tr.p.clone(), st[0].clone(), st[1].clone(), list(st[2]))
                o = tr.run(1, test=test, record=record)
                if not math.isfinite(float(o["loss"][0])):   # the device loops' rule: stop before the update
                    tr.p.copy_(keep[0])
                    st[0].copy_(keep[1])
                    st[1].copy_(keep[2])
                    st[2][:] = keep[3]
                    tr.history.pop()
                    tr._pver -= 1
                    self._stop(r, "loss_not_finite", stop)
                    break
                for key in ("loss", "loss_test") + (("grad", "p_before", "counts") if record else ()):
                    if o[key] is not None:
                        out[key][r, it] = o[key][0]
                done[r] = it + 1

    def _run_native(self, n_iters, test, chunk, record, forward, out, done, stop):
        hd = self.rhs.hd
        sv, _ = self._members[0]._fast_path()
        b1, b2 = self._members[0].opt.beta
        oc = self.solver.to_c()
        target = self.target.contiguous()
        call = hd.train_forward_ensemble_tsit5 if forward else hd.train_ensemble_tsit5
        B = self.u0.shape[0] if self.u0.dim() == 2 else 1
        if not forward and self.device_loop == "any" and hd.fit_ensemble_supported(B):
            call = hd.fit_ensemble_tsit5                      # (every small chain but the Lotka-Volterra shape)
        bps = self.bp
        keys = ("loss", "loss_test") + (("grad", "p_before", "counts") if record else ())
        at = 0
        while at < n_iters and self.live():
            live = self.live()
            k = min(n_iters - at, int(chunk) if chunk is not None else self.default_chunk(len(live)))
            # a stopped replica is left out of the launch: the live rows are gathered, and scattered back after it
            whole = len(live) == self.R
            idx = torch.as_tensor(live, device=self.p.device)
            p, m, v = (self.p, self.m, self.v) if whole else (x[idx].contiguous() for x in (self.p, self.m, self.v))
            res = call(p, m, v, self.u0, float(self.tspan[0]), float(self.tspan[1]), sv, target, oc,
                       [self.eta[r] for r in live], (b1, b2), self._members[0].opt.eps, [bps[r] for r in live], k,
                       test=test, record=record, l1=None if forward else [self.sparse_reg[r] for r in live])
            if not whole:
                for dst, src in ((self.p, p), (self.m, m), (self.v, v)):
                    dst[idx] = src
            host = {key: (res[key].cpu() if key in ("loss", "loss_test", "counts") and res[key] is not None
                          else res[key]) for key in keys}
            ran_through = all(d == k for d in res["iters_done"])
            if ran_through:                                   # (the usual case: whole blocks at once)
                for key in keys:
                    if host[key] is not None:
                        rows = idx.to(out[key].device)
                        out[key][rows, at:at + k] = host[key]
            losses = host["loss"].tolist()
            for j, r in enumerate(live):
                tr, d = self._members[r], int(res["iters_done"][j])
                bp = bps[r]
                for _ in range(d):                            # Flux's βp .*= β, once per iteration done
                    bp[0] *= b1
                    bp[1] *= b2
                tr._pver += d
                tr._drop_pre()
                tr.history.extend(losses[j][:d])
                if not ran_through:
                    for key in keys:
                        if host[key] is not None:
                            out[key][r, at:at + d] = host[key][j, :d]
                done[r] += d
                if res["stop"][j] != "ok":
                    self._stop(r, res["stop"][j], stop)
            at += k


class TrajectoryTrainer:
    """Training on R initial conditions where every trajectory is an ODE of its own (SciML's EnsembleProblem over u0
    under one loss): the ordinary way a NeuralODE is fitted to several experiments.  u0 is [R, N], target
    [len(saveat), R, N]; the loss is mse_loss over the whole tensor and its gradient the mean of the R batch-1
    gradients, each solve and adjoint with its own step control (adjoint.trajectories_mse_gradient: on the GPU one
    launch for all R where the handle covers the chain).  Trainer at the same matrix u0 solves ONE ODE over all R·N
    entries instead: one error norm, one step size, other step counts and so another gradient.

    loss_and_grad() adds the L1 term of sparse_reg on the host by Trainer's formula; step() is one Adam update
    (kanode_adam_step on the GPU) and raises KanodeError before it when any trajectory stopped, leaving p and the
    moments as they were.  One process: a data-parallel split over trajectories is not part of this class.
    f32 is passed to trajectories_mse_gradient: "device" runs float32 parameters on the fp32 one-launch entry where the
    handle covers the chain (off by default; a later change may flip it)."""

    def __init__(self, rhs, u0, tspan, saveat, target, p0, eta: float = 5e-4, solver: Tsit5Options | None = None,
                 sparse_reg: float = 0.0, f32: str = "host"):
        if not isinstance(u0, torch.Tensor) or u0.dim() != 2:
            raise ValueError("TrajectoryTrainer: u0 must be a tensor of shape [R, N]")
        self.f32 = f32   # what trajectories_mse_gradient does with float32 parameters ("host" / "device")
        self.rhs, self.u0, self.tspan, self.saveat, self.target = rhs, u0, tspan, saveat, target
        self.p = p0.detach().clone()
        self.opt = FusedAdam(eta) if self.p.is_cuda else Adam(eta)
        self.solver = solver or Tsit5Options()
        self.sparse_reg = sparse_reg
        self.history = []
        self.last_info = None   # info of the last loss_and_grad (path, stop, the step counts)

    def predict(self, p=None):
        """solve_trajectories at p (default: the current parameters)."""
        from .ode import solve_trajectories
        return solve_trajectories(self.rhs, self.u0, self.tspan, self.p if p is None else p, self.saveat, self.solver)

    def loss_and_grad(self):
        """(loss (0-dim tensor), gradient [P], info) at the current parameters."""
        from .adjoint import trajectories_mse_gradient
        loss, g, info = trajectories_mse_gradient(self.rhs, self.u0, self.tspan, self.p, self.saveat, self.target,
                                                  self.solver, f32=self.f32)
        self.last_info = info
        loss = torch.as_tensor(loss, dtype=g.dtype, device=g.device)
        if self.sparse_reg:   # (Trainer._with_l1's statements)
            p = self.p.detach()
            loss = loss + reg_loss(p, self.sparse_reg, 0.0)
            g = g + self.sparse_reg * torch.sign(p).reshape(g.shape)
        return loss, g, info

    def _step(self):
        from . import _lib as L
        loss, g, info = self.loss_and_grad()
        bad = [r for r, s in enumerate(info["stop"]) if s != "ok"]
        if bad:
            raise L.KanodeError(f"TrajectoryTrainer.step: trajectory {bad[0]} stopped ({info['stop'][bad[0]]}); "
                                f"{len(bad)} of {len(info['stop'])} stopped, the parameters are unchanged")
        self.opt.update(self.p, g.contiguous())
        lv = float(loss)
        self.history.append(lv)
        return lv, g

    def step(self) -> float:
        return self._step()[0]

    def run(self, n_iters: int, record: bool = False) -> dict:
        """n_iters iterations; {"loss": [...]} and, with record, "grad" and "p_before" (lists of tensors)."""
        out = {"loss": []}
        if record:
            out["grad"], out["p_before"] = [], []
        for _ in range(int(n_iters)):
            pb = self.p.detach().clone() if record else None
            lv, g = self._step()
            out["loss"].append(lv)
            if record:
                out["grad"].append(g.detach().clone())
                out["p_before"].append(pb)
        return out
