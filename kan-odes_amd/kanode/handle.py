"""Owning wrapper of a `kanode_handle*` — device tensors in, device tensors out.

Array convention: a Julia column-major [N, B] array (one trajectory contiguous)
is a C-contiguous torch tensor of shape (B, N): identical memory, so no copies
cross the boundary.  The flat parameter vector is the ComponentArray order
(include/kanode.h).  Every call is asynchronous on torch's current stream.
"""
from __future__ import annotations

import contextlib
import ctypes as C
from collections import namedtuple
from dataclasses import dataclass, field

import numpy as np
import torch

from . import _lib as L


@dataclass(frozen=True)
class LayerCfg:
    """One KDense layer's constructor arguments (kdense.jl:20-37)."""
    in_dims: int
    out_dims: int
    grid_len: int
    normalizer: str = "tanh_fast"
    basis: str = "rbf"
    use_base_act: bool = True
    grid_lims: tuple = (-1.0, 1.0)
    denominator: float | None = None
    iqf_reference_quirk: bool = True

    def to_c(self) -> L.LayerSpecC:
        if self.normalizer not in L.NORM:
            raise ValueError(f"normalizer {self.normalizer!r} not in {sorted(L.NORM)}")
        if self.basis not in L.BASIS:
            raise ValueError(f"basis_func {self.basis!r} not in {sorted(L.BASIS)}")
        den = 0.0 if self.denominator is None else float(np.float32(self.denominator))
        return L.LayerSpecC(self.in_dims, self.out_dims, self.grid_len, L.NORM[self.normalizer],
                            L.BASIS[self.basis], int(bool(self.use_base_act)),
                            float(np.float32(self.grid_lims[0])), float(np.float32(self.grid_lims[1])), den,
                            int(bool(self.iqf_reference_quirk)))

    @property
    def param_length(self) -> int:
        n = self.in_dims * self.grid_len * self.out_dims
        return n + (self.in_dims * self.out_dims if self.use_base_act else 0)


_DT = {torch.float32: L.F32, torch.float64: L.F64}

# kanode_last_fk_launch (include/kanode.h): out[0] indexes FK_FAMILIES
FK_FAMILIES = ("none", "pair_short", "pair_long", "wave_rhs", "stage", "step", "step_loop", "vjp", "vjp_stage",
               "adj_step_rows", "adj_step_wave", "adj_loop")
FkLaunch = namedtuple("FkLaunch", "family np norm path gt ni256 chunk grid combine fused_finish")


def _ptr(t: torch.Tensor | None):
    return None if t is None else C.c_void_p(t.data_ptr())


def _stream(device: torch.device):
    return C.c_void_p(torch.cuda.current_stream(device).cuda_stream)


class DenseOutput:
    """Owner of a kanode_solution* (the device-resident dense output of one solve)."""

    def __init__(self, hd):
        self.hd = hd
        self.ptr = C.c_void_p()

    @property
    def steps(self) -> int:
        return int(L.lib().kanode_solution_steps(self.ptr)) if self.ptr.value else 0

    def step_sizes(self):
        """(t_n, dt_n) of the accepted steps, float64 numpy arrays (kanode_solution_step_sizes)."""
        n = self.steps
        ts, dts = np.zeros(n), np.zeros(n)
        if n:
            L.lib().kanode_solution_step_sizes(self.ptr, ts.ctypes.data, dts.ctypes.data, n)
        return ts, dts

    def __del__(self):
        if getattr(self, "ptr", None) is not None and self.ptr.value:
            try:
                L.lib().kanode_solution_free(self.ptr)
            except Exception:
                pass
            self.ptr = C.c_void_p()


class KanodeHandle:
    """A configured RHS (chain or pointwise+periodic-Laplacian) bound to one device."""

    def __init__(self, layers, dtype=torch.float64, rhs_kind: str = "chain", nx: int = 0,
                 diffusion: float = 0.0, dx: float = 1.0, device=None):
        if dtype not in _DT:
            raise TypeError("dtype must be torch.float32 or torch.float64")
        layers = list(layers)
        if not 1 <= len(layers) <= L.MAX_LAYERS:
            raise ValueError(f"need 1..{L.MAX_LAYERS} layers")
        self.layers = layers
        self.dtype = dtype
        self.device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        spec = L.SpecC()
        spec.n_layers = len(layers)
        for i, lay in enumerate(layers):
            spec.layers[i] = lay.to_c()
        spec.dtype = _DT[dtype]
        spec.rhs_kind = {"chain": L.RHS_CHAIN, "pointwise_periodic_laplacian": L.RHS_POINTWISE_PERIODIC_LAPLACIAN}[rhs_kind]
        spec.nx = int(nx)
        spec.diffusion = float(diffusion)
        spec.dx = float(dx)
        spec.device = self.device.index or 0
        h = C.c_void_p()
        st = L.lib().kanode_create(C.byref(spec), C.byref(h))
        self._h = h
        if st != L.OK:
            msg = L.lib().kanode_last_error(h).decode() if h.value else ""
            L.lib().kanode_destroy(h)
            self._h = None
            raise L.KanodeError(f"kanode_create: {L.lib().kanode_status_string(st).decode()} ({msg})")
        self.rhs_kind = rhs_kind
        self.P = int(L.lib().kanode_param_length(h))
        self.N = int(L.lib().kanode_state_length(h))          # input state length
        self.N_out = self.N if rhs_kind != "chain" else layers[-1].out_dims
        self.layer_P = [int(L.lib().kanode_layer_param_length(h, i)) for i in range(len(layers))]
        self.layer_off = list(np.cumsum([0] + self.layer_P[:-1]))

    def __del__(self):
        h = getattr(self, "_h", None)
        if h is not None and h.value:
            try:
                L.lib().kanode_destroy(h)
            except Exception:
                pass
            self._h = None

    # -- helpers -----------------------------------------------------------
    def _check_t(self, t: torch.Tensor, shape, name: str) -> None:
        if not isinstance(t, torch.Tensor):
            raise TypeError(f"{name} must be a torch tensor")
        if t.device != self.device or t.dtype != self.dtype:
            raise TypeError(f"{name} must be {self.dtype} on {self.device}, got {t.dtype} on {t.device}")
        if not t.is_contiguous():
            raise ValueError(f"{name} must be contiguous")
        if shape is not None and tuple(t.shape) != tuple(shape):
            raise ValueError(f"{name} has shape {tuple(t.shape)}, expected {tuple(shape)}")

    def knots(self, layer: int = 0) -> np.ndarray:
        g = np.zeros(self.layers[layer].grid_len, np.float32)
        L.check(L.lib().kanode_knots(self._h, layer, C.c_void_p(g.ctypes.data)), self._h, "kanode_knots")
        return g

    def reserve(self, max_batch: int) -> None:
        L.check(L.lib().kanode_reserve(self._h, int(max_batch)), self._h, "kanode_reserve")

    @property
    def pointwise_table(self) -> bool:
        """POINTWISE rhs: kan1_.(u) through the per-launch polynomial table (kan_pp.hip)."""
        return L.lib().kanode_get_option(self._h, L.OPT_POINTWISE_TABLE) == 1

    @pointwise_table.setter
    def pointwise_table(self, on: bool) -> None:
        L.check(L.lib().kanode_set_option(self._h, L.OPT_POINTWISE_TABLE, 1 if on else 0), self._h,
                "kanode_set_option")

    def set_option(self, name: str, value: int) -> None:
        """kanode_set_option by name (include/kanode.h; the names are _lib.OPTIONS: pointwise_table,
        fused_step, fused_solve, fused_solve_cap, grid_rhs, grid_vjp, grid_adj_step, adj_step_rows, pair_vjp,
        pair_fuse, pair_persist, pair_persist_s, adj_fused_finish, pair_persist_max_wg, pair_persist_abort,
        fsens_wide, train_any_chain; last_adjoint and last_eval are read-only)."""
        if name not in L.OPTIONS:
            raise KeyError(f"unknown option {name!r}; known: {sorted(L.OPTIONS)}")
        L.check(L.lib().kanode_set_option(self._h, L.OPTIONS[name], int(value)), self._h, "kanode_set_option")

    def get_option(self, name: str) -> int:
        if name not in L.OPTIONS:
            raise KeyError(f"unknown option {name!r}; known: {sorted(L.OPTIONS)}")
        return int(L.lib().kanode_get_option(self._h, L.OPTIONS[name]))

    @contextlib.contextmanager
    def options(self, **kw):
        """Temporarily set options: `with hd.options(fused_step=0): ...`."""
        old = {k: self.get_option(k) for k in kw}
        try:
            for k, v in kw.items():
                self.set_option(k, v)
            yield self
        finally:
            for k, v in old.items():
                self.set_option(k, v)

    # -- RHS -----------------------------------------------------------------
    def rhs(self, p: torch.Tensor, u: torch.Tensor, out: torch.Tensor | None = None) -> torch.Tensor:
        """du (B, N_out) = f(u (B, N); p)."""
        B = u.shape[0] if u.dim() == 2 else 1
        self._check_t(p, (self.P,), "p")
        self._check_t(u, None, "u")
        if u.numel() != B * self.N:
            raise ValueError(f"u must hold B x {self.N} values, got shape {tuple(u.shape)}")
        shape = (B, self.N_out) if u.dim() == 2 else (self.N_out,)
        du = torch.empty(shape, dtype=self.dtype, device=self.device) if out is None else out
        self._check_t(du, shape, "du")
        L.check(L.lib().kanode_rhs(self._h, _ptr(p), _ptr(u), _ptr(du), B, _stream(self.device)), self._h,
                "kanode_rhs")
        return du

    @staticmethod
    def _stage_struct(ks, c, y_out=None, error=None) -> "L.StageC":
        if len(ks) != len(c) or len(ks) > L.MAX_STAGES:
            raise ValueError("ks and c must have equal length <= KANODE_MAX_STAGES")
        sg = L.StageC()
        sg.n_prev = len(ks)
        for j, (k, cj) in enumerate(zip(ks, c)):
            sg.k[j] = k.data_ptr()
            sg.c[j] = float(cj)
        if y_out is not None:
            sg.y_out = y_out.data_ptr()
        if error is not None:
            ec, abstol, reltol, sumsq = error
            if len(ec) != len(ks) + 1:
                raise ValueError("error coefficients need len(ks) + 1 entries")
            if sumsq.dtype != torch.float64 or sumsq.numel() < 1:
                raise ValueError("sumsq must be a float64 device tensor")
            sg.want_error = 1
            for j, e in enumerate(ec):
                sg.ec[j] = float(e)
            sg.abstol, sg.reltol = float(abstol), float(reltol)
            sg.error_sumsq = sumsq.data_ptr()
        return sg

    def vjp_stage(self, p, u, ks, c, lam, lks, lc, lam_out=None, error=None, dp=None):
        """Adjoint stage (kanode_vjp_stage): with y = u + Σ c_j k_j (forward dense output) and
        λs = lam + Σ lc_j lk_j (adjoint stage input, written to lam_out if given), returns
        (λsᵀ∂f/∂u at y, dp) with dp accumulated (+=) — a fresh zero vector when dp is None."""
        B = u.shape[0] if u.dim() == 2 else 1
        self._check_t(p, (self.P,), "p")
        for x, nm in [(u, "u"), (lam, "lam")] + [(k, "k") for k in ks] + [(k, "lk") for k in lks]:
            self._check_t(x, tuple(u.shape), nm)
        if lam_out is not None:
            self._check_t(lam_out, tuple(u.shape), "lam_out")
        if error is not None and error[3].device != self.device:
            raise ValueError("sumsq must live on the handle's device")
        su = self._stage_struct(ks, c)
        sl = self._stage_struct(lks, lc, lam_out, error)
        lamJ = torch.empty_like(u)
        if dp is None:
            dp = torch.zeros_like(p)
        L.check(L.lib().kanode_vjp_stage(self._h, _ptr(p), _ptr(u), C.byref(su), _ptr(lam), C.byref(sl), _ptr(lamJ),
                                         _ptr(dp), B, _stream(self.device)), self._h, "kanode_vjp_stage")
        return lamJ, dp

    def rhs_stage(self, p: torch.Tensor, u: torch.Tensor, ks, c, y_out: torch.Tensor | None = None,
                  error=None, out: torch.Tensor | None = None):
        """Runge-Kutta stage: du = f(u + Σ_j c_j k_j; p) (kanode_rhs_stage).

        ks: sequence of (B, N) tensors; c: their coefficients; y_out: optional tensor
        receiving the stage input; error: optional (ec, abstol, reltol, sumsq) with ec of
        len(ks)+1 coefficients and sumsq a 1-element float64 device tensor that receives
        Σ (e / (abstol + reltol·max(|u|,|y|)))², e = Σ ec_j k_j + ec_last du."""
        B = u.shape[0] if u.dim() == 2 else 1
        if len(ks) != len(c) or len(ks) > L.MAX_STAGES:
            raise ValueError("ks and c must have equal length <= KANODE_MAX_STAGES")
        self._check_t(p, (self.P,), "p")
        self._check_t(u, None, "u")
        for k in ks:
            self._check_t(k, tuple(u.shape), "k")
        du = torch.empty_like(u) if out is None else out
        self._check_t(du, tuple(u.shape), "du")
        sg = L.StageC()
        sg.n_prev = len(ks)
        for j, (k, cj) in enumerate(zip(ks, c)):
            sg.k[j] = k.data_ptr()
            sg.c[j] = float(cj)
        if y_out is not None:
            self._check_t(y_out, tuple(u.shape), "y_out")
            sg.y_out = y_out.data_ptr()
        if error is not None:
            ec, abstol, reltol, sumsq = error
            if len(ec) != len(ks) + 1:
                raise ValueError("error coefficients need len(ks) + 1 entries")
            if sumsq.dtype != torch.float64 or sumsq.device != self.device or sumsq.numel() < 1:
                raise ValueError("sumsq must be a float64 tensor on the handle's device")
            sg.want_error = 1
            for j, e in enumerate(ec):
                sg.ec[j] = float(e)
            sg.abstol, sg.reltol = float(abstol), float(reltol)
            sg.error_sumsq = sumsq.data_ptr()
        L.check(L.lib().kanode_rhs_stage(self._h, _ptr(p), _ptr(u), C.byref(sg), _ptr(du), B,
                                         _stream(self.device)), self._h, "kanode_rhs_stage")
        return du

    def vjp(self, p: torch.Tensor, u: torch.Tensor, lam: torch.Tensor, want_lamJ: bool = True,
            dp: torch.Tensor | None = None, accumulate_dp: bool = True):
        """(λᵀ∂f/∂u, Σ_b λᵀ∂f/∂p).  dp (if given) is ACCUMULATED into."""
        B = u.shape[0] if u.dim() == 2 else 1
        self._check_t(p, (self.P,), "p")
        self._check_t(u, None, "u")
        self._check_t(lam, (B, self.N_out) if u.dim() == 2 else (self.N_out,), "lam")
        lamJ = torch.empty_like(u) if want_lamJ else None
        if dp is None and accumulate_dp:
            dp = torch.zeros_like(p)
        L.check(L.lib().kanode_vjp(self._h, _ptr(p), _ptr(u), _ptr(lam), _ptr(lamJ), _ptr(dp), B,
                                   _stream(self.device)), self._h, "kanode_vjp")
        return lamJ, dp

    # -- integrator (kanode_solve_tsit5 / kanode_adjoint_tsit5) --------------------
    def solve_tsit5(self, p: torch.Tensor, u0: torch.Tensor, t0: float, tf: float, saveat, opts: "L.SolverOptsC",
                    keep_dense: bool = False):
        """Native Tsit5 solve on the device: (u_save (len(saveat), *u0.shape), stats dict,
        DenseOutput or None).  saveat: ascending floats within [t0, tf]."""
        B = u0.shape[0] if u0.dim() == 2 else 1
        self._check_t(p, (self.P,), "p")
        self._check_t(u0, None, "u0")
        if u0.numel() != B * self.N or self.N_out != self.N:
            raise ValueError("solve needs u0 of B x N entries and an RHS with N_in == N_out")
        sv = self._saveat_c(saveat)
        u_save = torch.empty((len(saveat),) + tuple(u0.shape), dtype=self.dtype, device=self.device)
        st = L.SolveStatsC()
        dense = None
        dptr = None
        if keep_dense:
            dense = self._dense_pool.pop() if getattr(self, "_dense_pool", None) else DenseOutput(self)
            dptr = C.byref(dense.ptr)
        L.check(L.lib().kanode_solve_tsit5(self._h, _ptr(p), _ptr(u0), B, float(t0), float(tf), sv, len(saveat),
                                           _ptr(u_save), C.byref(opts), dptr, C.byref(st), _stream(self.device)),
                self._h, "kanode_solve_tsit5")
        return u_save, dict(naccept=st.naccept, nreject=st.nreject, nf=st.nf), dense

    def solve_ensemble_supported(self, batch: int) -> bool:
        """kanode_solve_ensemble_supported: the ensemble solve covers this handle at `batch` trajectories (exactly
        where solve_tsit5 with control = auto runs as one workgroup)."""
        return bool(L.lib().kanode_solve_ensemble_supported(self._h, int(batch)))

    def solve_ensemble_tsit5(self, p: torch.Tensor, u0: torch.Tensor, t0: float, tf: float, saveat,
                             opts: "L.SolverOptsC"):
        """The solve of solve_tsit5 at every row of p [R, P] in one launch, one workgroup per replica
        (kanode_solve_ensemble_tsit5): (u_save (R, len(saveat), *u0.shape), stats (R dicts), stop (R names of
        _lib.SOLVE_STOP)).  u_save is pre-filled with NaN: a replica that reached maxiters ("maxiters", no
        exception) leaves the rows past its last reached stop that way.  An unsupported shape or a bad argument raises
        KanodeError."""
        B = u0.shape[0] if u0.dim() == 2 else 1
        if p.dim() != 2:
            raise ValueError("solve_ensemble_tsit5 needs p of shape [R, P]")
        R = int(p.shape[0])
        self._check_t(p, (R, self.P), "p")
        self._check_t(u0, None, "u0")
        if u0.numel() != B * self.N or self.N_out != self.N:
            raise ValueError("solve needs u0 of B x N entries and an RHS with N_in == N_out")
        sv = self._saveat_c(saveat)
        u_save = torch.full((R, len(saveat)) + tuple(u0.shape), float("nan"), dtype=self.dtype, device=self.device)
        st = (L.SolveStatsC * max(R, 1))()
        stop = (C.c_int32 * max(R, 1))()
        L.check(L.lib().kanode_solve_ensemble_tsit5(self._h, R, _ptr(p), _ptr(u0), B, float(t0), float(tf), sv,
                                                    len(saveat), _ptr(u_save), C.byref(opts), st, stop,
                                                    _stream(self.device)), self._h, "kanode_solve_ensemble_tsit5")
        stats = [dict(naccept=st[r].naccept, nreject=st[r].nreject, nf=st[r].nf) for r in range(R)]
        return u_save, stats, [L.SOLVE_STOP.get(int(stop[r]), str(stop[r])) for r in range(R)]

    def solve_trajectories_supported(self) -> bool:
        """kanode_solve_trajectories_supported: the trajectory solve covers this handle (a chain where solve_tsit5
        with control = auto runs as one workgroup at batch 1)."""
        return bool(L.lib().kanode_solve_trajectories_supported(self._h))

    def solve_trajectories_tsit5(self, p: torch.Tensor, u0: torch.Tensor, t0: float, tf: float, saveat,
                                 opts: "L.SolverOptsC"):
        """The solve of solve_tsit5 from every row of u0 [R, N] on its own, in one launch, a 16-lane row per
        trajectory (kanode_solve_trajectories_tsit5): every trajectory has its own error norm, step sizes and
        counters, where solve_tsit5 at u0 solves ONE ODE over all R·N entries.  Returns (u_save (len(saveat), R, N),
        stats (R dicts), stop (R names of _lib.SOLVE_STOP)).  u_save is pre-filled with NaN: a trajectory that
        reached maxiters ("maxiters", no exception) leaves its entries of the rows past its last reached stop that
        way.  An unsupported handle or a bad argument raises KanodeError."""
        self._check_t(p, (self.P,), "p")
        if u0.dim() != 2:
            raise ValueError("solve_trajectories_tsit5 needs u0 of shape [R, N]")
        R = int(u0.shape[0])
        self._check_t(u0, (R, self.N), "u0")
        if self.N_out != self.N:
            raise ValueError("solve needs an RHS with N_in == N_out")
        sv = self._saveat_c(saveat)
        u_save = torch.full((len(saveat), R, self.N), float("nan"), dtype=self.dtype, device=self.device)
        st = (L.SolveStatsC * max(R, 1))()
        stop = (C.c_int32 * max(R, 1))()
        L.check(L.lib().kanode_solve_trajectories_tsit5(self._h, _ptr(p), _ptr(u0), R, float(t0), float(tf), sv,
                                                        len(saveat), _ptr(u_save), C.byref(opts), st, stop,
                                                        _stream(self.device)), self._h,
                "kanode_solve_trajectories_tsit5")
        stats = [dict(naccept=st[r].naccept, nreject=st[r].nreject, nf=st[r].nf) for r in range(R)]
        return u_save, stats, [L.SOLVE_STOP.get(int(stop[r]), str(stop[r])) for r in range(R)]

    def trajectories_gradient_supported(self) -> bool:
        """kanode_trajectories_gradient_supported: the trajectory-ensemble gradient covers this handle (an fp64 chain
        of the one-workgroup solve at batch 1 whose column-group adjoint fits one workgroup; fused_solve on)."""
        return bool(L.lib().kanode_trajectories_gradient_supported(self._h))

    def trajectories_gradient_group(self, t0: float, tf: float, n_save: int, opts: "L.SolverOptsC") -> int:
        """kanode_trajectories_gradient_group: the trajectories trajectories_gradient_tsit5 puts into one launch for
        this problem (its buffer is capped at 256 MiB); more run as consecutive launch groups behind one call.
        0: not covered."""
        return int(L.lib().kanode_trajectories_gradient_group(self._h, float(t0), float(tf), int(n_save),
                                                              C.byref(opts)))

    def trajectories_gradient_tsit5(self, p: torch.Tensor, u0: torch.Tensor, t0: float, tf: float, saveat,
                                    target: torch.Tensor, opts: "L.SolverOptsC", rows: bool = False,
                                    du0: bool = False, u_save: bool = False):
        """mse_loss over the trajectories from every row of u0 [R, N] against target [len(saveat), R, N] and its
        gradient, every trajectory an ODE of its own with its own forward and adjoint step control, one workgroup each
        (kanode_trajectories_gradient_tsit5).  Returns (loss (float), dp [P], info): info holds "fwd_stats" and
        "adj_stats" (R dicts each), "stop" (R names of _lib.TRAIN_STOP) and, when asked, "dp_rows" [R, P] and
        "loss_rows" [R] (rows), "du0" [R, N], "u_save" [len(saveat), R, N] (pre-filled with NaN).  A trajectory that
        stops does not raise: stop[r] names the reason, its rows are NaN and so are loss and dp.  An unsupported handle
        or a bad argument raises KanodeError."""
        return self._trajectories_gradient("kanode_trajectories_gradient_tsit5", p, u0, t0, tf, saveat, target, opts,
                                           rows, du0, u_save)

    def _trajectories_gradient(self, _entry, p, u0, t0, tf, saveat, target, opts, rows, du0, u_save):
        """The call of either entry (the fp64 one or kanode_trajectories_gradient_f32_tsit5): same arguments."""
        self._check_t(p, (self.P,), "p")
        if u0.dim() != 2:
            raise ValueError("trajectories_gradient_tsit5 needs u0 of shape [R, N]")
        R = int(u0.shape[0])
        self._check_t(u0, (R, self.N), "u0")
        self._check_t(target, (len(saveat), R, self.N), "target")
        if self.N_out != self.N:
            raise ValueError("solve needs an RHS with N_in == N_out")
        sv = self._saveat_c(saveat)

        def new(*shape, fill=None):
            if fill is None:
                return torch.empty(shape, dtype=self.dtype, device=self.device)
            return torch.full(shape, fill, dtype=self.dtype, device=self.device)
        dp = new(self.P)
        out_rows = new(R, self.P) if rows else None
        out_loss = new(R) if rows else None
        out_du0 = new(R, self.N) if du0 else None
        out_us = new(len(saveat), R, self.N, fill=float("nan")) if u_save else None
        loss = C.c_double(float("nan"))
        fst = (L.SolveStatsC * max(R, 1))()
        ast = (L.SolveStatsC * max(R, 1))()
        stop = (C.c_int32 * max(R, 1))()
        L.check(getattr(L.lib(), _entry)(
            self._h, _ptr(p), _ptr(u0), R, float(t0), float(tf), sv, len(saveat), _ptr(target), C.byref(opts),
            C.byref(loss), _ptr(dp), _ptr(out_rows), _ptr(out_loss), _ptr(out_du0), _ptr(out_us), fst, ast,
            stop, _stream(self.device)), self._h, _entry)
        info = {"fwd_stats": [dict(naccept=fst[r].naccept, nreject=fst[r].nreject, nf=fst[r].nf) for r in range(R)],
                "adj_stats": [dict(naccept=ast[r].naccept, nreject=ast[r].nreject, nf=ast[r].nf) for r in range(R)],
                "stop": [L.TRAIN_STOP.get(int(stop[r]), str(stop[r])) for r in range(R)]}
        if rows:
            info["dp_rows"], info["loss_rows"] = out_rows, out_loss
        if du0:
            info["du0"] = out_du0
        if u_save:
            info["u_save"] = out_us
        return float(loss.value), dp, info

    def trajectories_gradient_f32_supported(self) -> bool:
        """kanode_trajectories_gradient_f32_supported: the fp32 trajectory-ensemble gradient covers this handle (an
        fp32 chain of the one-workgroup solve at batch 1 whose fp32 column-group adjoint fits one wave: P even;
        fused_solve on)."""
        return bool(L.lib().kanode_trajectories_gradient_f32_supported(self._h))

    def trajectories_gradient_f32_group(self, t0: float, tf: float, n_save: int, opts: "L.SolverOptsC") -> int:
        """kanode_trajectories_gradient_f32_group: trajectories_gradient_group for the fp32 entry.  0: not covered."""
        return int(L.lib().kanode_trajectories_gradient_f32_group(self._h, float(t0), float(tf), int(n_save),
                                                                  C.byref(opts)))

    def trajectories_gradient_f32_tsit5(self, p: torch.Tensor, u0: torch.Tensor, t0: float, tf: float, saveat,
                                        target: torch.Tensor, opts: "L.SolverOptsC", rows: bool = False,
                                        du0: bool = False, u_save: bool = False):
        """trajectories_gradient_tsit5 on an fp32 handle (kanode_trajectories_gradient_f32_tsit5): the same arguments
        and the same (loss, dp, info), every tensor float32; loss is the float total as a Python float."""
        return self._trajectories_gradient("kanode_trajectories_gradient_f32_tsit5", p, u0, t0, tf, saveat, target,
                                           opts, rows, du0, u_save)

    def _saveat_c(self, saveat):
        key = tuple(saveat)
        cache = self.__dict__.setdefault("_saveat_cache", {})
        sv = cache.get(key)
        if sv is None:   # (the C array of a saveat list, kept: training solves pass the same list every step)
            if len(cache) >= 16:
                cache.clear()
            sv = cache[key] = (C.c_double * max(1, len(saveat)))(*[float(x) for x in saveat])
        return sv

    def forward_sensitivity_supported(self, batch: int) -> bool:
        """kanode_forward_sensitivity_supported: the one-workgroup forward-sensitivity solve covers this batch."""
        return bool(L.lib().kanode_forward_sensitivity_supported(self._h, int(batch)))

    def forward_sensitivity_step_sizes(self):
        """(t_n, dt_n) of the accepted steps of the last forward_sensitivity_tsit5 (float64 numpy arrays)."""
        n = int(L.lib().kanode_forward_sensitivity_step_sizes(self._h, None, None, 0))
        ts, dts = np.zeros(max(n, 0)), np.zeros(max(n, 0))
        if n > 0:
            L.lib().kanode_forward_sensitivity_step_sizes(self._h, ts.ctypes.data, dts.ctypes.data, n)
        return ts, dts

    def forward_sensitivity_tsit5(self, p: torch.Tensor, u0: torch.Tensor, t0: float, tf: float, saveat,
                                  opts: "L.SolverOptsC"):
        """ForwardDiffSensitivity's solve (kanode_forward_sensitivity_tsit5): (u_save (n_save, *u0.shape),
        s_save (n_save, P, *u0.shape) = ∂u(saveat)/∂p, stats dict)."""
        B = u0.shape[0] if u0.dim() == 2 else 1
        self._check_t(p, (self.P,), "p")
        self._check_t(u0, None, "u0")
        if u0.numel() != B * self.N:
            raise ValueError("forward sensitivities need u0 of B x N entries")
        sv = self._saveat_c(saveat)
        u_save = torch.empty((len(saveat),) + tuple(u0.shape), dtype=self.dtype, device=self.device)
        s_save = torch.empty((len(saveat), self.P) + tuple(u0.shape), dtype=self.dtype, device=self.device)
        st = L.SolveStatsC()
        L.check(L.lib().kanode_forward_sensitivity_tsit5(self._h, _ptr(p), _ptr(u0), B, float(t0), float(tf), sv,
                                                         len(saveat), _ptr(u_save), _ptr(s_save), C.byref(opts),
                                                         C.byref(st), _stream(self.device)),
                self._h, "kanode_forward_sensitivity_tsit5")
        return u_save, s_save, dict(naccept=st.naccept, nreject=st.nreject, nf=st.nf)

    def adjoint_tsit5(self, p: torch.Tensor, dense: "DenseOutput", dl_du: torch.Tensor, opts: "L.SolverOptsC",
                      u_shape):
        """InterpolatingAdjoint over a kept forward solve: (dL/du0, dL/dp, stats)."""
        self._check_t(p, (self.P,), "p")
        self._check_t(dl_du, None, "dl_du")
        du0 = torch.empty(tuple(u_shape), dtype=self.dtype, device=self.device)
        dp = torch.empty_like(p)
        st = L.SolveStatsC()
        L.check(L.lib().kanode_adjoint_tsit5(self._h, _ptr(p), dense.ptr, _ptr(dl_du), _ptr(du0), _ptr(dp),
                                             C.byref(opts), C.byref(st), _stream(self.device)),
                self._h, "kanode_adjoint_tsit5")
        return du0, dp, dict(naccept=st.naccept, nreject=st.nreject, nf=st.nf)

    def train_supported(self, batch: int) -> bool:
        """kanode_train_supported: the device-resident training loop covers this handle at `batch` trajectories
        (one Lotka-Volterra trajectory; with the `train_any_chain` option on, every small fp64 chain of the
        one-workgroup solve and adjoint at up to 16 trajectories)."""
        return bool(L.lib().kanode_train_supported(self._h, int(batch)))

    def train_forward_supported(self, batch: int, with_test: bool = False) -> bool:
        """kanode_train_forward_supported: the device-resident Fisher-KPP loop on the forward-mode gradient covers this
        handle at `batch` trajectories (with_test: with the logged-loss solve as well)."""
        return bool(L.lib().kanode_train_forward_supported(self._h, int(batch), 1 if with_test else 0))

    def train_forward_tsit5(self, p, m, v, u0, t0: float, tf: float, saveat, target, opts: "L.SolverOptsC",
                            eta: float, beta, eps: float, beta_t, n_iters: int, test=None, record: bool = False):
        """train_tsit5 for a small Fisher-KPP field (kanode_train_forward_tsit5: the gradient by forward
        sensitivities): the same arguments and the same dict.  counts[:, :2] are the sensitivity solve's naccept and
        nreject; counts[:, 2:] those of the iteration's logged-loss solve when a test problem is given, else zero
        (there is no adjoint)."""
        return self._train("kanode_train_forward_tsit5", p, m, v, u0, t0, tf, saveat, target, opts, eta, beta, eps,
                           beta_t, n_iters, test, record)

    def set_l1_penalty(self, act_reg: float) -> None:
        """kanode_set_l1_penalty: λ of train_tsit5's loss term λ·Σ|p| (finite, >= 0; 0 = plain MSE)."""
        L.check(L.lib().kanode_set_l1_penalty(self._h, float(act_reg)), self._h, "kanode_set_l1_penalty")

    def get_l1_penalty(self) -> float:
        return float(L.lib().kanode_get_l1_penalty(self._h))

    def train_tsit5(self, p, m, v, u0, t0: float, tf: float, saveat, target, opts: "L.SolverOptsC", eta: float,
                    beta, eps: float, beta_t, n_iters: int, test=None, record: bool = False, l1: float = 0.0):
        """n_iters whole training iterations in one launch (kanode_train_tsit5): p, m, v are updated in place.
        test: None or (tf_test, saveat_test, target_test).  Returns a dict: loss (n_iters,), loss_test (n_iters,)
        or None, with record grad / p_before (n_iters, P) and counts (n_iters, 4), and iters_done, stop (a
        _lib.TRAIN_STOP name), error (the library's message when the loop stopped early, else None).  loss[it] is
        the loss at p_it, before the update; loss_test[it] at p_{it+1}.  An unsupported shape or a bad argument
        raises KanodeError; a stopped loop does not (the caller reads iters_done).
        l1: the weight λ of the sparsity term (loss + λ·Σ|p|, gradient + λ·sign(p)), set on the handle for this call
        and restored afterwards (so the call's penalty is always `l1`, whatever set_l1_penalty left there)."""
        old = self.get_l1_penalty()
        self.set_l1_penalty(l1)
        try:
            return self._train("kanode_train_tsit5", p, m, v, u0, t0, tf, saveat, target, opts, eta, beta, eps,
                               beta_t, n_iters, test, record)
        finally:
            self.set_l1_penalty(old)

    def _train(self, name, p, m, v, u0, t0, tf, saveat, target, opts, eta, beta, eps, beta_t, n_iters, test, record):
        """The call of train_tsit5 / train_forward_tsit5 (the two entries share their signature)."""
        B = u0.shape[0] if u0.dim() == 2 else 1
        for t, nm in ((p, "p"), (m, "m"), (v, "v")):
            self._check_t(t, (self.P,), nm)
        self._check_t(u0, None, "u0")
        if u0.numel() != B * self.N:
            raise ValueError("train_tsit5 needs u0 of B x N entries")
        self._check_t(target, (len(saveat),) + tuple(u0.shape), "target")
        n = int(n_iters)
        kw = dict(dtype=torch.float64, device=self.device)
        loss = torch.zeros(n, **kw)
        tf_t, sv_t, n_t, tg_t, loss_t = 0.0, None, 0, None, None
        if test is not None:
            tf_t, sat, tg_t = test
            self._check_t(tg_t, (len(sat),) + tuple(u0.shape), "target_test")
            sv_t, n_t = self._saveat_c(sat), len(sat)
            loss_t = torch.zeros(n, **kw)
        grad = torch.zeros((n, self.P), **kw) if record else None
        pb = torch.zeros((n, self.P), **kw) if record else None
        counts = torch.zeros((n, 4), dtype=torch.int64, device=self.device) if record else None
        done, stop = C.c_int64(0), C.c_int32(0)
        st = getattr(L.lib(), name)(self._h, _ptr(p), _ptr(m), _ptr(v), _ptr(u0), B, float(t0), float(tf),
                                    self._saveat_c(saveat), len(saveat), _ptr(target), float(tf_t), sv_t, n_t,
                                    _ptr(tg_t), C.byref(opts), float(eta), float(beta[0]), float(beta[1]),
                                    float(eps), float(beta_t[0]), float(beta_t[1]), n, _ptr(loss), _ptr(loss_t),
                                    _ptr(grad), _ptr(pb), _ptr(counts), C.byref(done), C.byref(stop),
                                    _stream(self.device))
        err = None
        if st != L.OK:
            if stop.value == 0:
                L.check(st, self._h, name)
            err = L.lib().kanode_last_error(self._h).decode()
        return dict(loss=loss, loss_test=loss_t, grad=grad, p_before=pb, counts=counts, iters_done=int(done.value),
                    stop=L.TRAIN_STOP.get(int(stop.value), str(stop.value)), error=err)

    def train_ensemble_tsit5(self, p, m, v, u0, t0: float, tf: float, saveat, target, opts: "L.SolverOptsC", eta,
                             beta, eps: float, beta_t, n_iters: int, test=None, record: bool = False, l1=None):
        """train_tsit5 on R independent replicas in one launch, one workgroup each (kanode_train_ensemble_tsit5):
        p, m, v are [R, P] and updated in place, eta and l1 (None: all zero) sequences of R floats, beta_t R pairs
        of running powers.  Returns train_tsit5's dict with a leading replica dimension on loss, loss_test, grad,
        p_before and counts; iters_done and stop are lists of R; error is the library's text naming the lowest
        stopped replica, or None.  A replica that stops does not raise and does not hold up the others."""
        return self._train_ensemble("kanode_train_ensemble_tsit5", p, m, v, u0, t0, tf, saveat, target, opts, eta, l1,
                                    beta, eps, beta_t, n_iters, test, record)

    def train_forward_ensemble_tsit5(self, p, m, v, u0, t0: float, tf: float, saveat, target, opts: "L.SolverOptsC",
                                     eta, beta, eps: float, beta_t, n_iters: int, test=None, record: bool = False,
                                     l1=None):
        """train_ensemble_tsit5 for a small Fisher-KPP field (kanode_train_forward_ensemble_tsit5); a non-zero
        entry of l1 raises "not supported"."""
        return self._train_ensemble("kanode_train_forward_ensemble_tsit5", p, m, v, u0, t0, tf, saveat, target, opts,
                                    eta, l1, beta, eps, beta_t, n_iters, test, record)

    def fit_ensemble_supported(self, batch: int) -> bool:
        """kanode_fit_ensemble_supported: fit_ensemble_tsit5 covers this handle at `batch` trajectories: exactly the
        shapes train_supported gains with `train_any_chain` on (the option is not read), never the Lotka-Volterra
        shape (train_ensemble_tsit5's)."""
        return bool(L.lib().kanode_fit_ensemble_supported(self._h, int(batch)))

    def fit_ensemble_group(self, batch: int, t0: float, tf: float, n_save: int, n_save_test: int,
                           opts: "L.SolverOptsC") -> int:
        """kanode_fit_ensemble_group: the replicas fit_ensemble_tsit5 puts into one launch for this problem (its
        256 MiB cap on the handle's buffer; more replicas run in consecutive groups of this size), 0 where the
        problem is not covered or does not fit one workgroup's LDS."""
        return int(L.lib().kanode_fit_ensemble_group(self._h, int(batch), float(t0), float(tf), int(n_save),
                                                     int(n_save_test), C.byref(opts)))

    def fit_ensemble_tsit5(self, p, m, v, u0, t0: float, tf: float, saveat, target, opts: "L.SolverOptsC", eta,
                           beta, eps: float, beta_t, n_iters: int, test=None, record: bool = False, l1=None):
        """train_ensemble_tsit5 for every other small fp64 chain (kanode_fit_ensemble_tsit5: a pruned [2,k,2], a
        [3,6,3] chain, three layers, up to 16 trajectories): the same arguments and the same dict; replica r equals
        train_tsit5 with `train_any_chain` on, bit for bit.  The Lotka-Volterra shape raises "not supported"."""
        return self._train_ensemble("kanode_fit_ensemble_tsit5", p, m, v, u0, t0, tf, saveat, target, opts, eta, l1,
                                    beta, eps, beta_t, n_iters, test, record)

    def _train_ensemble(self, name, p, m, v, u0, t0, tf, saveat, target, opts, eta, l1, beta, eps, beta_t, n_iters,
                        test, record):
        B = u0.shape[0] if u0.dim() == 2 else 1
        if p.dim() != 2 or p.shape[0] < 1:
            raise ValueError("train_ensemble_tsit5 needs p, m, v of shape [R, P]")
        R = int(p.shape[0])
        for t, nm in ((p, "p"), (m, "m"), (v, "v")):
            self._check_t(t, (R, self.P), nm)
        self._check_t(u0, None, "u0")
        if u0.numel() != B * self.N:
            raise ValueError("train_ensemble_tsit5 needs u0 of B x N entries")
        self._check_t(target, (len(saveat),) + tuple(u0.shape), "target")
        eta = [float(e) for e in eta]
        bt = [float(x) for pair in beta_t for x in pair]
        if len(eta) != R or len(bt) != 2 * R or (l1 is not None and len(l1) != R):
            raise ValueError("train_ensemble_tsit5 needs R entries of eta, l1 and beta_t")
        c_eta = (C.c_double * R)(*eta)
        c_bt = (C.c_double * (2 * R))(*bt)
        c_l1 = None if l1 is None else (C.c_double * R)(*[float(x) for x in l1])
        n = int(n_iters)
        kw = dict(dtype=torch.float64, device=self.device)
        loss = torch.zeros((R, n), **kw)
        tf_t, sv_t, n_t, tg_t, loss_t = 0.0, None, 0, None, None
        if test is not None:
            tf_t, sat, tg_t = test
            self._check_t(tg_t, (len(sat),) + tuple(u0.shape), "target_test")
            sv_t, n_t = self._saveat_c(sat), len(sat)
            loss_t = torch.zeros((R, n), **kw)
        grad = torch.zeros((R, n, self.P), **kw) if record else None
        pb = torch.zeros((R, n, self.P), **kw) if record else None
        counts = torch.zeros((R, n, 4), dtype=torch.int64, device=self.device) if record else None
        done, stop = (C.c_int64 * R)(), (C.c_int32 * R)()
        L.check(getattr(L.lib(), name)(self._h, R, _ptr(p), _ptr(m), _ptr(v), _ptr(u0), B, float(t0), float(tf),
                                       self._saveat_c(saveat), len(saveat), _ptr(target), float(tf_t), sv_t, n_t,
                                       _ptr(tg_t), C.byref(opts), c_eta, c_l1, float(beta[0]), float(beta[1]),
                                       float(eps), c_bt, n, _ptr(loss), _ptr(loss_t), _ptr(grad), _ptr(pb),
                                       _ptr(counts), done, stop, _stream(self.device)), self._h, name)
        err = L.lib().kanode_last_error(self._h).decode() if any(s != 0 for s in stop) else None
        return dict(loss=loss, loss_test=loss_t, grad=grad, p_before=pb, counts=counts, iters_done=list(done),
                    stop=[L.TRAIN_STOP.get(int(s), str(s)) for s in stop], error=err)

    def table_rejections(self):
        """Intervals the last table builds rejected: (φ, φ', swish), -1 for a table not built yet
        (kanode_table_rejections; their points take the direct formula)."""
        out = (C.c_int32 * 3)()
        L.check(L.lib().kanode_table_rejections(self._h, out), self._h, "kanode_table_rejections")
        return tuple(int(x) for x in out)

    def last_fk_launch(self):
        """The handle's last Fisher-KPP table launch (kanode_last_fk_launch): an FkLaunch of family (a name of
        FK_FAMILIES), np, norm ("softsign", "tanh_fast", "runtime"), path ("rec", "rec_corr" or None), gt, ni256,
        chunk, grid, combine, fused_finish."""
        out = (C.c_int32 * 8)()
        L.check(L.lib().kanode_last_fk_launch(self._h, out), self._h, "kanode_last_fk_launch")
        v = [int(x) for x in out]
        return FkLaunch(FK_FAMILIES[v[0]], v[1], {2: "softsign", 0: "tanh_fast", -1: "runtime"}[v[2]],
                        {-1: None, 1: "rec", 2: "rec_corr"}[v[3]], v[4], bool(v[5] & 1), v[6], v[7], (v[5] >> 1) & 3,
                        bool(v[5] & 8))

    def adjoint_step_sizes(self):
        """The accepted step sizes of the last adjoint_tsit5 (option record_adjoint_steps; else empty)."""
        n = int(L.lib().kanode_adjoint_step_sizes(self._h, None, 0))
        hs = np.zeros(max(n, 0))
        if n > 0:
            L.lib().kanode_adjoint_step_sizes(self._h, hs.ctypes.data, n)
        return hs

    def release_dense(self, dense: "DenseOutput") -> None:
        """Return a dense output's device storage for reuse by the next solve."""
        if not hasattr(self, "_dense_pool"):
            self._dense_pool = []
        if dense is not None and dense.ptr.value and len(self._dense_pool) < 2:
            self._dense_pool.append(dense)

    # -- single layer ----------------------------------------------------------
    def layer_forward(self, layer: int, p_layer: torch.Tensor, x: torch.Tensor) -> torch.Tensor:
        cfg = self.layers[layer]
        K = x.shape[0]
        self._check_t(p_layer, (cfg.param_length,), "p_layer")
        self._check_t(x, (K, cfg.in_dims), "x")
        y = torch.empty((K, cfg.out_dims), dtype=self.dtype, device=self.device)
        L.check(L.lib().kanode_layer_forward(self._h, layer, _ptr(p_layer), _ptr(x), _ptr(y), K,
                                             _stream(self.device)), self._h, "kanode_layer_forward")
        return y

    def layer_forward_stage(self, layer: int, p_layer: torch.Tensor, x: torch.Tensor, ks, c, y_out=None,
                            lam=None, lks=(), lc=(), ls_out=None) -> torch.Tensor:
        """kanode_layer_forward_stage: the layer at y = x + Σ c_j k_j (-> y_out if given) and, with lam,
        λs = lam + Σ lc_j lk_j -> ls_out (required then); returns the layer output (K, O)."""
        cfg = self.layers[layer]
        K = x.shape[0]
        self._check_t(p_layer, (cfg.param_length,), "p_layer")
        for a, nm in [(x, "x")] + [(k, "k") for k in ks] + ([(y_out, "y_out")] if y_out is not None else []):
            self._check_t(a, (K, cfg.in_dims), nm)
        if lam is not None:
            if ls_out is None:
                raise ValueError("layer_forward_stage: lam needs ls_out")
            for a, nm in [(lam, "lam"), (ls_out, "ls_out")] + [(k, "lk") for k in lks]:
                self._check_t(a, (K, cfg.in_dims), nm)
        sx = self._stage_struct(ks, c, y_out)
        sl = self._stage_struct(lks, lc, ls_out) if lam is not None else None
        y = torch.empty((K, cfg.out_dims), dtype=self.dtype, device=self.device)
        L.check(L.lib().kanode_layer_forward_stage(self._h, layer, _ptr(p_layer), _ptr(x), C.byref(sx), _ptr(lam),
                                                   C.byref(sl) if sl is not None else None, _ptr(y), K,
                                                   _stream(self.device)), self._h, "kanode_layer_forward_stage")
        return y

    def layer_vjp(self, layer: int, p_layer: torch.Tensor, x: torch.Tensor, ybar: torch.Tensor):
        cfg = self.layers[layer]
        K = x.shape[0]
        self._check_t(p_layer, (cfg.param_length,), "p_layer")
        self._check_t(x, (K, cfg.in_dims), "x")
        self._check_t(ybar, (K, cfg.out_dims), "ybar")
        xbar = torch.empty_like(x)
        pbar = torch.zeros_like(p_layer)
        L.check(L.lib().kanode_layer_vjp(self._h, layer, _ptr(p_layer), _ptr(x), _ptr(ybar), _ptr(xbar), _ptr(pbar),
                                         K, _stream(self.device)), self._h, "kanode_layer_vjp")
        return xbar, pbar

    def edge_activations(self, layer: int, p_layer: torch.Tensor, x: torch.Tensor) -> torch.Tensor:
        """act (K, I, O) with act[k, i, o] = φ_{o,i}(x[k, i]) (Activation_getter.jl:28-31,48-53)."""
        cfg = self.layers[layer]
        K = x.shape[0]
        self._check_t(p_layer, (cfg.param_length,), "p_layer")
        self._check_t(x, (K, cfg.in_dims), "x")
        act = torch.empty((K, cfg.in_dims, cfg.out_dims), dtype=self.dtype, device=self.device)
        L.check(L.lib().kanode_edge_activations(self._h, layer, _ptr(p_layer), _ptr(x), _ptr(act), K,
                                                _stream(self.device)), self._h, "kanode_edge_activations")
        return act

    def edge_scores(self, layer: int, p_layer: torch.Tensor, x: torch.Tensor) -> torch.Tensor:
        """scores (I, O) with scores[i, o] = max_k |φ_{o,i}(x[k, i])| (kanode_edge_scores: what the reference's prune
        reads from activation_getter, LV_driver_KANODE.jl:79-80), without the (K, I, O) array and for any out_dims.
        A NaN activation makes its edge's score NaN."""
        cfg = self.layers[layer]
        K = x.shape[0]
        self._check_t(p_layer, (cfg.param_length,), "p_layer")
        self._check_t(x, (K, cfg.in_dims), "x")
        scores = torch.empty((cfg.in_dims, cfg.out_dims), dtype=self.dtype, device=self.device)
        L.check(L.lib().kanode_edge_scores(self._h, layer, _ptr(p_layer), _ptr(x), _ptr(scores), K,
                                           _stream(self.device)), self._h, "kanode_edge_scores")
        return scores
