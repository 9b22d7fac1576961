"""The ForwardDiffSensitivity Dual solve restated on the CPU, for fields of several trajectories.

`dual_tsit5` is the restatement of tests/test_gpu_fsens.py (third-party semantics, restated from the pinned
SciMLSensitivity 7.69 / DiffEqBase / OrdinaryDiffEq 6.89 -- verify where Julia exists) in numpy over the stacked state
z = [u; S_1..S_P] (rows) with the B·Nx entries in columns, extended by a forced first step (`opt.dt` with
`adaptive`) and a fixed step (`adaptive=False`).  Its right-hand side (`dual_rhs`) is built from the CPU oracle
alone: oracle.fk_rhs for f(u), oracle.fk_vjp for J S_k (J = D lap + diag φ'(u) is symmetric, so λᵀJ = J λ) and the
closed form ∂φ/∂C_k = B_k(N(u)), ∂φ/∂W = swish(u).  No HIP code sits inside it.

`problem(Nx, B, G)` is the family of small periodic fields the wide forward-sensitivity tests run on; SHAPES lists
the five shapes and FORCED the three forced-first-step cases whose first steps the controller rejects."""
import math
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "kan-odes_amd")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

from kanode.ode import A, BTILDE, Tsit5Options, interp_weights  # noqa: E402
from oracle import oracle as O  # noqa: E402

# (Nx, B, G): 78 entries, the third trajectory straddles entry 64 (table path) / 89: odd Nx (formula path), the
# automatic rule's limit / 65: one entry in the upper half / 128: the kernel's cap, a periodic wrap lands on the half
# boundary / 94 entries with G = 5 (7 waves)
SHAPES = [(26, 3, 10), (89, 1, 10), (13, 5, 10), (64, 2, 10), (47, 2, 5)]
# (Nx, B, G, first step): the restatement rejects 2, 3 and 2 steps
FORCED = [(26, 3, 10, 0.5), (13, 5, 10, 0.5), (89, 1, 10, 1.0)]
# accepted steps of the C port and of the restatement, each on its own steps (no rejection), by reltol
COUNTS = {1e-3: [11, 8, 12, 9, 10], 1e-6: [21, 16, 25, 17, 23]}
D, DX, T, SAVEAT = 0.01, 0.04, 1.0, [0.0, 0.3, 0.55, 1.0]


def initial_conditions(Nx: int, B: int) -> np.ndarray:
    x = np.arange(Nx) / Nx
    u0 = np.zeros((B, Nx))
    for b in range(B):
        c, w, a = (0.3 + 0.2 * b) % 1.0, 0.12 + 0.03 * b, 0.9 - 0.15 * b
        d = np.minimum(np.abs(x - c), 1.0 - np.abs(x - c))
        u0[b] = a * np.exp(-(d / w) ** 2) + 0.02 * b
    return u0


def params(G: int, draw: int = 0) -> np.ndarray:
    """G = 10: bench.fk_trained_like_params() + default_rng(3).normal(0, 0.05, 11); the four G = 10 shapes of SHAPES
    take consecutive draws of that one generator, in table order (`draw` = the shape's index: the recorded step
    counts COUNTS and the rejections of FORCED belong to these draws).  G = 5: default_rng(5).normal(0, 0.3, 6)."""
    if G == 10:
        import bench
        rng = np.random.default_rng(3)
        noise = [rng.normal(0.0, 0.05, 11) for _ in range(draw + 1)][draw]
        return bench.fk_trained_like_params() + noise
    assert G == 5
    return np.random.default_rng(5).normal(0.0, 0.3, 6)


_problems = {}


def problem(Nx: int, B: int, G: int) -> dict:
    key = (Nx, B, G)
    if key not in _problems:
        draw = SHAPES.index(key) if key in SHAPES and G == 10 else 0
        _problems[key] = dict(Nx=Nx, B=B, G=G, P=G + 1, D=D, dx=DX, T=T, tspan=(0.0, T), saveat=list(SAVEAT),
                              u0=initial_conditions(Nx, B), p=params(G, draw), spec=O.LayerSpec(1, 1, G, "softsign"))
    return _problems[key]


def dual_rhs(pr: dict):
    """F([u; S]) = [f(u); J S_k + ∂f/∂p_k] over z of shape (1 + P, B·Nx)."""
    spec, p, B, Nx, P = pr["spec"], pr["p"], pr["B"], pr["Nx"], pr["P"]
    g = O.knots(spec).astype(np.float64)
    invh = float(O.inv_h(spec))

    def F(z):
        u = np.ascontiguousarray(z[0].reshape(B, Nx))
        du = O.fk_rhs(spec, p, pr["D"], pr["dx"], u)
        uu = np.ascontiguousarray(np.broadcast_to(u, (P, B, Nx)).reshape(P * B, Nx))
        jS, _ = O.fk_vjp(spec, p, pr["D"], pr["dx"], uu, np.ascontiguousarray(z[1:].reshape(P * B, Nx)))
        n = u / (1.0 + np.abs(u))
        basis = np.exp(-((n[None] - g[:, None, None]) * invh) ** 2)
        dfdp = np.concatenate([basis, (u / (1.0 + np.exp(-u)))[None]], 0)
        return np.concatenate([du.reshape(1, -1), (jS.reshape(P, B, Nx) + dfdp).reshape(P, -1)], 0)
    return F


def initial_state(pr: dict) -> np.ndarray:
    return np.concatenate([pr["u0"].reshape(1, -1), np.zeros((pr["P"], pr["B"] * pr["Nx"]))], 0)


def dual_tsit5(F, z0, t0, tf, saveat, opt: Tsit5Options, replay=None):
    """The Dual-number Tsit5 solve on z = [u; S_1..S_P] (rows), entries in columns.  Returns (z at saveat, naccept,
    nreject).  replay: take these accepted step sizes in order (another solver's sequence; nothing is rejected)."""
    numel = z0.size

    def nrm(z):   # per entry: sqrt(value² + Σ partials²)
        return np.sqrt((z * z).sum(0))

    def rmsn(x):
        return math.sqrt(float((x * x).sum()) / numel)

    out, si = [], 0
    while si < len(saveat) and saveat[si] <= t0 + 1e-14 * max(1.0, abs(t0)):
        out.append(z0)
        si += 1
    z, t = z0, t0
    k1 = F(z)
    if not opt.adaptive or opt.dt is not None:
        dt = float(opt.dt)
    else:   # Hairer & Wanner over the Dual state
        sk = opt.abstol + nrm(z0) * opt.reltol
        d0, d1 = rmsn(z0 / sk), rmsn(k1 / sk)
        dt0 = 1e-6 if (d0 < 1e-5 or d1 < 1e-5) else 0.01 * d0 / d1
        dt0 = min(dt0, tf - t0)
        f1 = F(z0 + dt0 * k1)
        d2 = rmsn((f1 - k1) / sk) / dt0
        mx = max(d1, d2)
        dt1 = max(1e-6, dt0 * 1e-3) if mx <= 1e-15 else (0.01 / mx) ** (1.0 / 5.0)
        dt = min(100 * dt0, dt1, tf - t0)
    qold, naccept, nreject = opt.qoldinit, 0, 0
    for _ in range(100000):
        if t >= tf - 1e-14 * max(1.0, abs(tf)):
            break
        if replay is not None:
            dt = float(replay[naccept])
        dt = min(dt, tf - t)
        ks = [k1]
        for i in range(6):
            y = z
            for j, a in enumerate(A[i]):
                y = y + (dt * a) * ks[j]
            ks.append(F(y))
        znew = y
        dtnew = dt
        if opt.adaptive:
            e = sum((dt * b) * k for b, k in zip(BTILDE, ks))
            skn = opt.abstol + np.maximum(nrm(z), nrm(znew)) * opt.reltol
            EEst = rmsn(e / skn)
            q11 = EEst ** opt.beta1 if EEst > 0 else 0.0
            if EEst > 1.0 and replay is None:
                nreject += 1
                dt = dt / min(1.0 / opt.qmin, q11 / opt.gamma)
                continue
            q = q11 / (qold ** opt.beta2)
            q = max(1.0 / opt.qmax, min(1.0 / opt.qmin, q / opt.gamma))
            dtnew = dt / q
            qold = max(EEst, opt.qoldinit)
        tn = t + dt
        while si < len(saveat) and saveat[si] <= tn + 1e-12 * max(1.0, abs(tn)):
            ts = saveat[si]
            if abs(ts - tn) <= 1e-12 * max(1.0, abs(tn)):
                out.append(znew)
            else:
                w = interp_weights((ts - t) / dt)
                out.append(z + dt * sum(wi * k for wi, k in zip(w, ks)))
            si += 1
        z, k1, t = znew, ks[6], tn
        naccept += 1
        dt = dtnew
    return np.stack(out), naccept, nreject


def restate(pr: dict, opt: Tsit5Options, replay=None):
    """(u (n_save, B, Nx), S (n_save, P, B, Nx), naccept, nreject) of the restatement on `pr`."""
    z, na, nr = dual_tsit5(dual_rhs(pr), initial_state(pr), 0.0, pr["T"], pr["saveat"], opt, replay=replay)
    ns, B, Nx, P = z.shape[0], pr["B"], pr["Nx"], pr["P"]
    return z[:, 0].reshape(ns, B, Nx), z[:, 1:].reshape(ns, P, B, Nx), na, nr


_cport = {}


def c_port(pr: dict, tol: float):
    """oracle.fk_fsens_solve on `pr` at reltol = tol, abstol = tol·1e-3 (computed once per problem and tolerance):
    (u, S, stats)."""
    key = (pr["Nx"], pr["B"], pr["G"], tol)
    if key not in _cport:
        u, S, st, _ = O.fk_fsens_solve(pr["spec"], pr["p"], pr["D"], pr["dx"], pr["u0"], pr["T"], pr["saveat"],
                                       abstol=tol * 1e-3, reltol=tol)
        u.setflags(write=False)
        S.setflags(write=False)
        _cport[key] = (u, S, st)
    return _cport[key]


def worst(u, S, u_ref, S_ref):
    """(max |u - u_ref| over max(1, max|u_ref|), max over k of max |S_k - S_ref_k| over max |S_ref_k|)."""
    eu = float(np.abs(u - u_ref).max()) / max(1.0, float(np.abs(u_ref).max()))
    es = 0.0
    for k in range(S_ref.shape[1]):
        sc = max(float(np.abs(S_ref[:, k]).max()), 1e-300)
        es = max(es, float(np.abs(S[:, k] - S_ref[:, k]).max()) / sc)
    return eu, es
