"""The cases the parity matrix of the per-point Fisher-KPP kernels shares (test_fk_cases_cpu.py,
test_gpu_fk_matrix.py): the table of records, the kernel instantiation and launch class each record is meant to reach
(kan_fk.hip: fk_rhs_kernel / fk_vjp_kernel behind launch_fk_rhs / launch_fk_vjp / fk_rhs_go / fk_vjp_go, the path
from make_layer_const in kanode_abi.cpp), its seeded inputs, the error scale, and the numpy models the CPU test holds
against the oracle.  No tests live here.

The pass criterion everywhere is gpu_util.assert_close(got, ref, scale, gpu_util.RTOL[dtype]).  The scale is
layer_cases.layer_error_scale of the [1, 1] layer at the B·nx points (y, x̄ per point, p̄ summed over the points),
plus the Laplacian's Σ|terms| |co|·(|u₋| + 2|u| + |u₊|) for du and the same on |λ| for λᵀJ (with the reference
matrix's Nx = 1 and Nx = 2 rows).  The reference of an fp32 record is the fp64 oracle at the fp32-rounded inputs.

fk_path, fk_instantiation and fk_launch_class restate the C++ rules and can drift from them: the records state their
classes by hand, test_fk_cases_cpu.py holds them against these restatements, and the GPU matrix reaches a class only
through the library's own rule."""
from __future__ import annotations

import zlib
from dataclasses import dataclass
from types import SimpleNamespace

import numpy as np

import layer_cases as LC
from oracle import kanode_np as N
from oracle import oracle as O

DIRECT, REC, REC_CORR = "direct", "rec", "rec_corr"
K_BLOCK, K_GRID_CAP, K_SLAB_BLOCKS, K_MAX_GRID = 256, 4096, 4096, 32      # kan_common.hpp, kanode_options.hpp
NORM_RANGE = {"tanh_fast": (-1.0, 1.0), "tanh": (-1.0, 1.0), "softsign": (-1.0, 1.0), "sigmoid": (0.0, 1.0),
              "sigmoid_fast": (0.0, 1.0)}                               # (identity: unbounded)


# ---- the classification, restated -------------------------------------------------------------------------------
def layer_consts(spec):
    """make_layer_const's recurrence constants in float64 (kanode_abi.cpp:43-105): s, gs, δ, τ_c, Δ_j, e_j, K_j."""
    G = spec.grid_len
    grid = N.knots(G, *spec.grid_lims)
    den = N.default_denominator(G) if spec.denominator is None else np.float32(spec.denominator)
    invh = N.inv_h(den)
    sd, g0 = float(invh), float(grid[0])
    lo, hi = float(np.float32(spec.grid_lims[0])), float(np.float32(spec.grid_lims[1]))
    delta = (hi - lo) * sd / (G - 1)
    bounded = spec.normalizer in NORM_RANGE
    nlo, nhi = NORM_RANGE.get(spec.normalizer, (-1.0, 1.0))
    zlo, zhi = (nlo - g0) * sd, (nhi - g0) * sd
    tau_c = (zlo + zhi) if bounded else 0.0
    Dl = (grid.astype(np.float64) - g0) * sd
    e = Dl - np.arange(G, dtype=np.float64) * delta
    DL = Dl.astype(np.longdouble)
    K = (np.exp(-DL * DL) * np.exp(np.longdouble(tau_c) * e.astype(np.longdouble))).astype(np.float64)
    return SimpleNamespace(grid=grid, invh=invh, s=sd, g0=g0, gs=-g0 * sd, delta=delta, tau_c=tau_c, Dl=Dl, e=e, K=K,
                           bounded=bounded, zlo=zlo, zhi=zhi)


def fk_path(dtype, spec):
    """The basis path make_layer_const picks: the recurrence for a bounded normalizer with rbf when
    zmax² <= lim, 2·zmax·|δ|·(G-1) <= lim (lim = 600 in fp64, 80 in fp32), δ > 0 and max|τ'e_j| = (zhi - zlo)·max|e_j|
    <= 1e-5 (fp64) / 1e-3 (fp32); REC when every e_j is 0, else REC_CORR; everything else DIRECT."""
    c = layer_consts(spec)
    if spec.basis != "rbf" or not c.bounded:
        return DIRECT
    zmax = max(abs(c.zlo), abs(c.zhi))
    lim = 600.0 if dtype == "f64" else 80.0
    emax = float(np.max(np.abs(c.e)))
    tmax = (c.zhi - c.zlo) * emax
    ok = (zmax * zmax <= lim and 2.0 * zmax * abs(c.delta) * (spec.grid_len - 1) <= lim and c.delta > 0.0
          and tmax <= (1e-5 if dtype == "f64" else 1e-3))
    if not ok:
        return DIRECT
    return REC if emax == 0.0 else REC_CORR


SPECIALISED = [("softsign", REC_CORR, 10), ("softsign", REC, 5), ("tanh_fast", REC, 5)]
RUNTIME = [("runtime", REC_CORR, 0), ("runtime", REC, 0), ("runtime", DIRECT, 0)]


def fk_instantiation(dtype, spec):
    """(NORM, PATH, GT) of launch_fk_rhs / launch_fk_vjp: one of the three specialised triples, else the runtime
    kernel of the path (GT = 0: the loops predicated to kMaxGrid)."""
    t = (spec.normalizer, fk_path(dtype, spec), spec.grid_len)
    return t if t in SPECIALISED else ("runtime", t[1], 0)


def fk_launch_class(nx):
    """("pair" / "odd", "short" / "long", tpt_log2) of fk_rhs_go: pairs of points for an even nx; one unit per thread
    while units <= kBlock, else the long-grid kernel's loop (the VJP kernel always loops; it takes a second trip in
    the long class only)."""
    pair = nx % 2 == 0
    units = nx // 2 if pair else nx
    m, tl = min(units, K_BLOCK), 0
    while (1 << tl) < m:
        tl += 1
    return ("pair" if pair else "odd", "short" if units <= K_BLOCK else "long", tl)


def fk_grid_stride(nx, B):
    """(rhs, vjp): whether the trajectory loop `b += bstride` takes a second trip (grid capped at kGridCap /
    KAN_SLAB_BLOCKS blocks of kBlock >> tpt_log2 trajectories)."""
    tpb = K_BLOCK >> fk_launch_class(nx)[2]
    blocks = (B + tpb - 1) // tpb
    return blocks > K_GRID_CAP, blocks > K_SLAB_BLOCKS


# ---- variants -----------------------------------------------------------------------------------------------------
# name: (normalizer, basis, G, grid limits, denominator, iqf quirk, base term, path in fp64, path in fp32)
_L = (-1.0, 1.0)
VARIANTS = {
    "softsign_rbf_G3": ("softsign", "rbf", 3, _L, None, True, True, REC, REC),
    "softsign_rbf_G5": ("softsign", "rbf", 5, _L, None, True, True, REC, REC),
    "softsign_rbf_G7": ("softsign", "rbf", 7, _L, None, True, True, REC_CORR, REC_CORR),
    "softsign_rbf_G10": ("softsign", "rbf", 10, _L, None, True, True, REC_CORR, DIRECT),
    "tanhfast_rbf_G3": ("tanh_fast", "rbf", 3, _L, None, True, True, REC, REC),
    "tanhfast_rbf_G5": ("tanh_fast", "rbf", 5, _L, None, True, True, REC, REC),
    "tanhfast_rbf_G6": ("tanh_fast", "rbf", 6, _L, None, True, True, REC_CORR, REC_CORR),
    "tanhfast_rbf_G10": ("tanh_fast", "rbf", 10, _L, None, True, True, REC_CORR, DIRECT),
    "tanh_rbf_G3": ("tanh", "rbf", 3, _L, None, True, True, REC, REC),
    "tanh_rbf_G5": ("tanh", "rbf", 5, _L, None, True, True, REC, REC),
    "tanh_rbf_G7": ("tanh", "rbf", 7, _L, None, True, True, REC_CORR, REC_CORR),
    "tanh_rbf_G10": ("tanh", "rbf", 10, _L, None, True, True, REC_CORR, DIRECT),
    "sigmoidfast_rbf_G9": ("sigmoid_fast", "rbf", 9, _L, None, True, True, REC, DIRECT),
    "sigmoid_rbf_01_G5": ("sigmoid", "rbf", 5, (0.0, 1.0), None, True, True, REC, REC),
    "softsign_rbf_den_G5": ("softsign", "rbf", 5, _L, 0.4, True, True, REC, REC),              # δ = 1.25
    "identity_rbf_G5_nobase": ("identity", "rbf", 5, _L, None, True, False, DIRECT, DIRECT),
    "tanh_rswaf_G5": ("tanh", "rswaf", 5, _L, None, True, True, DIRECT, DIRECT),
    "softsign_iqf_quirk_G5": ("softsign", "iqf", 5, _L, None, True, True, DIRECT, DIRECT),
    "softsign_iqf_exact_G5": ("softsign", "iqf", 5, _L, None, False, True, DIRECT, DIRECT),
    "softsign_rbf_G2": ("softsign", "rbf", 2, _L, None, True, True, REC, REC),
    "softsign_rbf_G32": ("softsign", "rbf", 32, _L, None, True, True, DIRECT, DIRECT),
    "softsign_rbf_G5_nobase": ("softsign", "rbf", 5, _L, None, True, False, REC, REC),
    "softsign_rbf_G7_nobase": ("softsign", "rbf", 7, _L, None, True, False, REC_CORR, REC_CORR),
}
# the long, the kBlock-edge and the grid-stride shapes: every instantiation of either dtype (so one variant per PATH)
EDGE_VARIANTS = ["softsign_rbf_G5", "softsign_rbf_G7", "softsign_rbf_G10", "tanh_rswaf_G5", "tanhfast_rbf_G5",
                 "tanh_rbf_G3"]
STRIDE_VARIANTS = {"f64": ["softsign_rbf_G5", "softsign_rbf_G10", "tanh_rswaf_G5"],
                   "f32": ["softsign_rbf_G5", "softsign_rbf_G7", "softsign_rbf_G10"]}

# nx: the launch class stated by hand (pair / odd, short / long, tpt_log2) and what the shape is there for
SHAPES = {
    1: ("odd", "short", 0),        # lap3's Nx == 1 row
    2: ("pair", "short", 0),       # lap3's Nx == 2 rows inside a pair
    3: ("odd", "short", 2),        # the smallest generic row; one idle lane
    4: ("pair", "short", 1),       # lap_pair from Nx >= 4
    5: ("odd", "short", 3),
    26: ("pair", "short", 4),      # 13 units on 16 lanes (the reference's Nx)
    255: ("odd", "short", 8),      # units = kBlock - 1
    257: ("odd", "long", 8),       # units = kBlock + 1: a second trip of the q-loop for one lane
    512: ("pair", "short", 8),     # units = kBlock exactly
    514: ("pair", "long", 8),      # units = kBlock + 1 pairs
}
SMALL_NX, EDGE_NX = (1, 2, 3, 4, 5, 26), (255, 257, 512, 514)
STRIDE_NX, STRIDE_B = 257, 4099      # tpb = 1: 4099 blocks wanted, both caps are 4096

# diffusion: name -> (D, dx) of nx.  "D0": the KAN part alone; "Ddx2": the Laplacian coefficient is 1, so neither part
# masks the other; "Dref": the reference's D = 0.01 on [0, 1]; "Dneg": the Allen-Cahn sign and spacing
DIFFUSION = {
    "D0": lambda nx: (0.0, 1.0 / max(nx - 1, 1)),
    "Ddx2": lambda nx: ((1.0 / max(nx - 1, 1)) ** 2, 1.0 / max(nx - 1, 1)),
    "Dref": lambda nx: (0.01, 1.0 / max(nx - 1, 1)),
    "Dneg": lambda nx: (-1e-4, 0.05),
}


@dataclass(frozen=True)
class Case:
    variant: str
    dtype: str      # "f64" / "f32"
    nx: int
    B: int
    diff: str       # a key of DIFFUSION

    @property
    def id(self):
        return f"{self.variant}-{self.dtype}-nx{self.nx}-B{self.B}-{self.diff}"

    @property
    def seed(self):
        return zlib.crc32(self.id.encode())

    @property
    def G(self):
        return VARIANTS[self.variant][2]

    @property
    def use_base(self):
        return VARIANTS[self.variant][6]

    @property
    def path(self):
        """The path this record is meant to reach (stated by hand in VARIANTS)."""
        return VARIANTS[self.variant][7 if self.dtype == "f64" else 8]

    @property
    def instantiation(self):
        t = (VARIANTS[self.variant][0], self.path, self.G)
        return t if t in SPECIALISED else ("runtime", self.path, 0)

    @property
    def launch(self):
        return SHAPES[self.nx]

    @property
    def grid_stride(self):
        return self.nx == STRIDE_NX and self.B == STRIDE_B

    @property
    def D_dx(self):
        return DIFFUSION[self.diff](self.nx)

    @property
    def table_off(self):
        """An fp64 handle is created with the pointwise table off, so that an even-nx rbf / rswaf record reaches
        kan_fk.hip (fp32, odd nx and iqf never take the table)."""
        return self.dtype == "f64"

    @property
    def claims(self):
        """What of REQUIRED this record covers."""
        out = {("inst",) + self.instantiation, ("path", self.path, self.use_base),
               ("launch",) + self.launch[:2]}
        if self.grid_stride:
            out |= {("stride", "rhs"), ("stride", "vjp")}
        return out

    def spec(self):
        n, b, G, lims, den, quirk, base, _, _ = VARIANTS[self.variant]
        return O.LayerSpec(1, 1, G, n, b, base, lims, den, quirk)

    def np_dtype(self):
        return np.float64 if self.dtype == "f64" else np.float32

    def data(self):
        """(p, u, λ) in float64, an fp32 record's values rounded to fp32 first.  Glorot-uniform parameters, u uniform
        in [-3, 3], λ standard normal; planted into u at seeded places, as far as the record has room beside one
        random point: exactly 0, +1e4 and -1e4 (the normalizer saturates, swish is x or 0) and, for identity, 7.0
        (16 knot widths off the grid)."""
        rng = np.random.default_rng(self.seed)
        G = self.G
        lim = np.sqrt(6.0 / (1 + G))
        parts = [rng.uniform(-lim, lim, G)]
        if self.use_base:
            parts.append(rng.uniform(-np.sqrt(3.0), np.sqrt(3.0), 1))
        p = np.concatenate(parts)
        u = rng.uniform(-3.0, 3.0, (self.B, self.nx))
        lam = rng.normal(size=(self.B, self.nx))
        plant = [0.0, 1e4, -1e4] + ([7.0] if VARIANTS[self.variant][0] == "identity" else [])
        k = min(len(plant), u.size - 1)
        if k > 0:
            u.reshape(-1)[rng.choice(u.size, k, replace=False)] = plant[:k]
        dt = self.np_dtype()
        return tuple(a.astype(dt).astype(np.float64) for a in (p, u, lam))


def _cases():
    out = []
    for dt in ("f64", "f32"):
        for diff in ("D0", "Ddx2"):
            for v in VARIANTS:
                for nx in SMALL_NX:
                    for B in (1, 5):
                        out.append(Case(v, dt, nx, B, diff))
            for v in EDGE_VARIANTS:
                for nx in EDGE_NX:
                    for B in (1, 5):
                        out.append(Case(v, dt, nx, B, diff))
            for v in STRIDE_VARIANTS[dt]:
                out.append(Case(v, dt, STRIDE_NX, STRIDE_B, diff))
        for v in ("softsign_rbf_G10", "softsign_rbf_G5", "tanh_rswaf_G5"):
            for nx in (26, 257):
                out.append(Case(v, dt, nx, 5, "Dref"))
        out.append(Case("softsign_rbf_G10", dt, 26, 5, "Dneg"))
    return out


CASES = _cases()


def _required(dt):
    inst = [t for t in SPECIALISED + RUNTIME if not (dt == "f32" and t == ("softsign", REC_CORR, 10))]
    return ({("inst",) + t for t in inst} | {("path", pth, b) for pth in (DIRECT, REC, REC_CORR) for b in (True, False)}
            | {("launch", a, b) for a in ("pair", "odd") for b in ("short", "long")}
            | {("stride", "rhs"), ("stride", "vjp")})


# what the table has to reach, per dtype (test_fk_cases_cpu.py: each claimed by a record whose claim the restated
# rules confirm).  fp32 cannot reach softsign·REC_CORR·10: G = 10 is DIRECT there (2·(G-1)² = 162 > 80).
REQUIRED = {dt: _required(dt) for dt in ("f64", "f32")}


# ---- the Laplacian and the error scale ---------------------------------------------------------------------------
def lap_apply(v, cd, co, mut=None):
    """Rows of the reference's (D·lap)·v for v (B, nx): periodic tridiagonal; at nx = 2 the corner coincides with the
    off-diagonal, at nx = 1 it overwrote the diagonal (Fisher-KPP_Source.jl:55-59).  mut: "no_wrap" (the last
    point's right neighbour is itself, index nx-1, not 0), "generic_small" (nx = 1, 2 as a generic row: the corner is
    counted twice)."""
    nx = v.shape[1]
    if nx == 1:
        return co * v + cd * v + co * v if mut == "generic_small" else co * v
    if nx == 2:
        if mut == "generic_small":
            return cd * v + co * v[:, ::-1] + co * v[:, ::-1]
        return cd * v + co * v[:, ::-1]
    vm, vp = np.roll(v, 1, axis=1), np.roll(v, -1, axis=1)
    if mut == "no_wrap":
        vp[:, -1] = v[:, -1]
    return co * vm + cd * v + co * vp


def fk_error_scale(case, p, u, lam):
    """(du, λᵀJ, dp) scales: layer_cases.layer_error_scale of the [1, 1] layer at the B·nx points plus the Laplacian's
    Σ|terms| on |u| and on |λ|."""
    D, dx = case.D_dx
    cd, co = N.fk_coeffs(D, dx)
    ys, xs, ps = LC.layer_error_scale(case.spec(), p, u.reshape(-1, 1), lam.reshape(-1, 1))
    return (ys.reshape(u.shape) + lap_apply(np.abs(u), abs(cd), abs(co)),
            xs.reshape(u.shape) + lap_apply(np.abs(lam), abs(cd), abs(co)), ps)


def oracle(case, p, u, lam):
    """(du, λᵀJ, dp) of the fp64 C oracle."""
    D, dx = case.D_dx
    lamJ, dp = O.fk_vjp(case.spec(), p, D, dx, u, lam)
    return O.fk_rhs(case.spec(), p, D, dx, u), lamJ, dp


# ---- the numpy model and its wrong restatements ----------------------------------------------------------------
def skipped_points(case):
    """The points a kernel that ran only the first trip of the q-loop would miss (q >= tpt)."""
    pair, _, tl = case.launch
    i = np.arange(case.nx)
    return (i // 2 if pair == "pair" else i) >= (1 << tl)


def np_base(case, p, u, lam):
    """(kan, x̄, p̄) of oracle/kanode_np.py's [1, 1] layer at the points: what np_fk builds on (a caller may keep it)."""
    L = LC.np_layers([case.spec()])[0]
    x = u.reshape(-1, 1)
    xb, pb = L.vjp(p, x, lam.reshape(-1, 1))
    return L.fwd(p, x).reshape(u.shape), xb.reshape(u.shape), pb


def np_fk(case, p, u, lam, mut=None, base=None):
    """(du, λᵀJ, dp) of oracle/kanode_np.py's layer with this module's Laplacian, in float64.  mut names one wrong
    restatement: "no_wrap", "generic_small" (lap_apply); "exact_knots" (float64-exact knots g0 + j·δ/s in place of the
    Float32 LinRange knots: the e_j correction dropped); "no_base_second" (the base term missing on the second point
    of every pair); "dw_slot" (dW left at slot GL: dp[G] = 0); "skip_q" (points with q >= tpt not computed);
    "first_trip" (trajectories past the first trip of the b-loop not computed).  base: np_base of the same inputs."""
    spec = case.spec()
    G = case.G
    D, dx = case.D_dx
    cd, co = N.fk_coeffs(D, dx)
    L = LC.np_layers([spec])[0]
    if mut == "exact_knots":
        c = layer_consts(spec)
        L.grid = c.g0 + np.arange(G, dtype=np.float64) * c.delta / c.s
        x = u.reshape(-1, 1)
        xb, pb = L.vjp(p, x, lam.reshape(-1, 1))
        kan, xb = L.fwd(p, x).reshape(u.shape), xb.reshape(u.shape)
    else:
        kan, xb, pb = np_base(case, p, u, lam) if base is None else base
    lmut = mut if mut in ("no_wrap", "generic_small") else None
    du = lap_apply(u, cd, co, lmut) + kan
    lamJ = lap_apply(lam, cd, co, lmut) + xb
    pb = pb.copy()
    if mut == "no_base_second" and case.use_base and case.nx % 2 == 0:
        second = np.broadcast_to((np.arange(case.nx) % 2 == 1)[None, :], u.shape)
        W = p[G]
        du = du - np.where(second, W * N.swish(u), 0.0)
        lamJ = lamJ - np.where(second, W * lam * N.dswish(u), 0.0)
        pb[G] -= np.sum(np.where(second, lam * N.swish(u), 0.0))
    if mut == "dw_slot" and case.use_base:
        pb[G] = 0.0
    dead = None
    if mut == "skip_q":
        dead = np.broadcast_to(skipped_points(case)[None, :], u.shape)
    elif mut == "first_trip":
        tpb = K_BLOCK >> case.launch[2]
        dead = np.broadcast_to((np.arange(case.B) >= K_GRID_CAP * tpb)[:, None], u.shape)
    if dead is not None:      # p̄ is linear in λ: take the dead points' share out
        pb -= L.vjp(p, u[dead].reshape(-1, 1), lam[dead].reshape(-1, 1))[1]
        du, lamJ = np.where(dead, 0.0, du), np.where(dead, 0.0, lamJ)
    return du, lamJ, pb


# name: the records of the mutation's group
MUTATIONS = {
    "no_wrap": lambda c: c.nx >= 3 and c.D_dx[0] != 0.0,
    "generic_small": lambda c: c.nx <= 2 and c.D_dx[0] != 0.0,
    "exact_knots": lambda c: c.dtype == "f64" and c.path == REC_CORR,
    "no_base_second": lambda c: c.use_base and c.nx % 2 == 0,
    "dw_slot": lambda c: c.use_base and c.G < K_MAX_GRID,
    "skip_q": lambda c: c.launch[1] == "long",
    "first_trip": lambda c: c.grid_stride,
}


# ---- two fp32 restatements (the bar has to hold them: test_fk_cases_cpu.py) -----------------------------------------
def c_oracle_f32(case, p, u, lam):
    """The fp32 C oracle: O.layer_fwd / O.layer_vjp in fp32 per trajectory plus a numpy fp32 Laplacian; the
    trajectories' dp summed pairwise in fp32 (one serial fp32 sum over 10^6 points would lose what no kernel
    loses: they sum per thread, per block and per slab row)."""
    f = np.float32
    spec = case.spec()
    D, dx = case.D_dx
    cd, co = (f(v) for v in N.fk_coeffs(D, dx))
    p32, u32, l32 = p.astype(f), u.astype(f), lam.astype(f)
    kan = O.layer_fwd(spec, p32, u32.reshape(-1, 1)).reshape(u.shape)
    xb = np.empty_like(u32)
    pbs = np.empty((p.size, case.B), f)
    for b in range(case.B):
        x, pb = O.layer_vjp(spec, p32, u32[b].reshape(-1, 1), l32[b].reshape(-1, 1))
        xb[b], pbs[:, b] = x.reshape(-1), pb
    du = lap_apply(u32, cd, co) + kan
    lamJ = lap_apply(l32, cd, co) + xb
    assert du.dtype == f and lamJ.dtype == f
    return du, lamJ, np.sum(pbs, axis=1, dtype=f)


def _fma32(a, b, c):
    """fp32 fma: the product of two fp32 values is exact in float64."""
    return (np.asarray(a, np.float64) * np.asarray(b, np.float64) + np.asarray(c, np.float64)).astype(np.float32)


def rec_model_f32(case, p, u, lam):
    """The recurrence as kan_device.hpp / kan_fk.hip state it, in numpy fp32 (REC and REC_CORR records): rec_anchor
    with the split square (z0² = p2 + perr, E0 = fma(-E, perr, E)), R = exp(2·z0·δ), τ' = 2·z0 - τ_c; kan11_fwd's
    three Horner sweeps in R over A_j = C_j K_j, C_j K_j e_j, C_j K_j e_j²/2; kan11_vjp's forward product F·R^j with
    the per-knot correction fma(τ', fma(τ', KQ_j, KE_j), K_j), Σ C_j z_j φ_j = z0·sa - sb."""
    f = np.float32
    spec, G, corr = case.spec(), case.G, case.path == REC_CORR
    assert case.path in (REC, REC_CORR)
    c = layer_consts(spec)
    D, dx = case.D_dx
    cd, co = (f(v) for v in N.fk_coeffs(D, dx))
    x, l = u.reshape(-1).astype(f), lam.reshape(-1).astype(f)
    C = p[:G].astype(f)
    s, gs, delta, tau_c, invh = f(c.s), f(c.gs), f(c.delta), f(c.tau_c), f(c.invh)
    K, e, Dl = c.K.astype(f), c.e.astype(f), c.Dl.astype(f)
    q = f(0.5) * e * e
    n = N.NORMS[spec.normalizer](x).astype(f)
    z0 = _fma32(n, s, gs)
    p2 = z0 * z0
    perr = _fma32(z0, z0, -p2)
    E = np.exp(-p2)
    E0 = _fma32(-E, perr, E)
    tw = z0 + z0
    R = np.exp(tw * delta)
    taup = tw - tau_c
    A, Bq, Q = C * K, C * K * e, C * K * q
    s0, s1, s2 = (np.full_like(x, v[G - 1]) for v in (A, Bq, Q))
    for j in range(G - 2, -1, -1):
        s0 = _fma32(s0, R, A[j])
        if corr:
            s1, s2 = _fma32(s1, R, Bq[j]), _fma32(s2, R, Q[j])
    kan = E0 * _fma32(taup, _fma32(taup, s2, s1), s0) if corr else E0 * s0
    KE, KQ, CD = K * e, K * q, C * Dl
    F, sa, sb = E0, np.zeros_like(x), np.zeros_like(x)
    dp = []
    for j in range(G):
        kc = _fma32(taup, _fma32(taup, KQ[j], KE[j]), K[j]) if corr else K[j]
        phi = F * kc
        dp.append(np.sum(l * phi, dtype=f))
        sa, sb = _fma32(C[j], phi, sa), _fma32(CD[j], phi, sb)
        F = F * R
    xb = ((f(-2) * invh) * l * _fma32(z0, sa, -sb)) * N.dnorm(spec.normalizer, x, n).astype(f)
    if case.use_base:
        W = f(p[G])
        sg = N.sigmoid(x).astype(f)
        om = x * sg
        kan = kan + W * om
        xb = xb + (W * l) * (om + sg * (f(1) - om))
        dp.append(np.sum(l * om, dtype=f))
    du = lap_apply(u.astype(f), cd, co) + kan.reshape(u.shape)
    lamJ = lap_apply(lam.astype(f), cd, co) + xb.reshape(u.shape)
    assert du.dtype == f and lamJ.dtype == f
    return du, lamJ, np.array(dp, f)
