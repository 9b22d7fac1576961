"""The cases the wide-layer / mixed-class parity matrix shares (test_layer_cases_cpu.py, test_gpu_layer_matrix.py):
the table of records, the kernel class each record is meant to reach, its seeded inputs, and a first-order
rounding-error scale of y, x̄ and p̄ built on oracle/kanode_np.py in float64.  No tests live here.

The pass criterion everywhere is gpu_util.assert_close(got, ref, scale, gpu_util.RTOL[dtype]) with the scale of
error_scale / layer_error_scale; the two RTOL values are the project's stated ones.

error_scale, per layer (x the layer input, dx the error scale of x: 0 for the chain input, the previous layer's
y scale for a hidden layer; n = normalizer(x), a = (n - knot)·invh, φ the basis value, ψ the factor the basis
pullback multiplies C^T ȳ with):
  n_err   = |n| + |n'|·dx                          rounding of n, and the input's error through n'
  a_err   = invh·(n_err + |knot|)                  rounding of n - knot and of the product, amplified by invh
  φ_s     = |φ|_terms + |φ'|·a_err                 |φ|_terms = φ, but 1 + tanh² for rswaf (1 - tanh² cancels: it
                                                   loses absolute, not relative, accuracy)
  ψ_s     = |ψ|_terms + |ψ'|·a_err
  swish_s = |swish| + |swish'|·dx,   swish'_s = |Ω| + σ·(1 + |Ω|) + |swish''|·dx
  n'_s    = the Ω-form derivative's term magnitudes + |dn'/dn|·n_err
  y_s     = Σ |C|·φ_s + Σ |W|·swish_s
  C̄_s    = Σ_k |ȳ|·φ_s,   W̄_s = Σ_k |ȳ|·swish_s
  x̄_s    = (Σ_g ψ_s·(Σ_o |C|·|ȳ|)·invh)·n'_s + (Σ_o |W|·|ȳ|)·swish'_s
Within one layer at exact inputs (dx = 0) the products of these term magnitudes are kept as they stand (they are the
single-layer scale).  Across layers the scale is first order in the propagated errors: of the expressions above only
the part linear in dx is kept (their derivative in dx at 0), and the error scale dȳ of a hidden cotangent (the next
layer's x̄ scale) goes through the plain magnitudes, |J|ᵀ·dȳ with |ψ|, |n'|, |swish'|, |φ|, |swish|, not through the
widened ones; products of two propagated errors are dropped.
Every output gets the floor gpu_util.chain_scale uses, + 1e-3·max (p̄: per layer).

Two chain scales come out of this.  chain_error_scale is for a chain result against the ORACLE: the hidden values
differ, so every hidden layer carries its worst-case Σ|terms| forward error through the next layer's |J|.  That
compounds: in fp32 a 1 % error of x̄ stays inside it on 150 of the 388 multi-layer records and an x̄ of all zeros on
16 (it is a statement of what fp32 can promise in the worst case, not a check that tells a wrong λᵀJ from a right one
there; in fp64 it is 5e7 times finer and does).  composition_error_scale is for a
chain result against the composition of the layer calls ON THE SAME DEVICE, where the hidden values are the same
bits (dx = 0 everywhere) and only the cotangent's rounding travels down: it stays near Σ|terms| of x̄ and is the
discriminating chain check (test_layer_cases_cpu.py holds a 1 % error of x̄ and of layer 0's p̄ against it)."""
from __future__ import annotations

import zlib
from dataclasses import dataclass

import numpy as np

from oracle import kanode_np as N
from oracle import oracle as O

COL, WIDE_IN, WIDE_OUT = "column", "wide-in", "wide-out"


def kernel_class(I, O_, G, use_base, esize):
    """The class kanode_create gives a layer (kanode_abi.cpp:209-223), restated: column when O <= 16, the
    (G·I + O + I)·65 staging fits 150 KiB and P <= 64·32; else wide-in when O <= 16 (kWideOMax); else wide-out when
    (G·I + I)·8 (kWideKT) elements fit 150 KiB; else None (refused).  This restatement can drift from the C++:
    the records state their classes by hand and test_layer_cases_cpu.py holds them against it, and the GPU
    matrix reaches a class only through the library's own rule."""
    P = O_ * G * I + (O_ * I if use_base else 0)
    if O_ <= 16 and (G * I + O_ + I) * 65 * esize <= 150 * 1024 and P <= 64 * 32:
        return COL
    if O_ <= 16:
        return WIDE_IN
    if (G * I + I) * 8 * esize <= 150 * 1024:
        return WIDE_OUT
    return None


def widein_slots(I, O_, G):
    """(tn, cw, nv, nw) of the wide-in forward (kan_kernels.hpp widein_cw, kan_wide.hip launch_kd_fwd_widein): the
    launch takes the (MV, MW) = (8, 2) kernel when nv <= 8 and nw <= 2, (16, 4) when nv <= 16 and nw <= 4, else
    (32, 8).  Like kernel_class this is a restatement that can drift from the C++ (kWIMaxV = 32, kWIMaxW = 8,
    kWideInMaxInputs = 64, kWideInMinChunks = 16 are written out); it only tells the CPU test which instantiation a
    record is expected to reach."""
    tn = (256 // O_) * O_
    cw = min((32 * tn) // (O_ * G), 64)
    if cw * O_ > 8 * tn:
        cw = (8 * tn) // O_
    if I >= 32 * 16:
        cw = min(cw, (I + 15) // 16)
    cw = max(cw, 1)
    return tn, cw, (O_ * G * cw + tn - 1) // tn, (O_ * cw + tn - 1) // tn


def widein_instantiation(I, O_, G):
    _, _, nv, nw = widein_slots(I, O_, G)
    return (8, 2) if nv <= 8 and nw <= 2 else ((16, 4) if nv <= 16 and nw <= 4 else (32, 8))


# ---- variants -----------------------------------------------------------------------------------------------
# name: (normalizer of layer 0, of the later layers, basis, grid limits, quirk, base: "all" / "none" / "first")
VARIANTS = {
    "tanhfast_rbf": ("tanh_fast", "tanh_fast", "rbf", (-1.0, 1.0), True, "all"),
    "tanh_rswaf": ("tanh", "tanh", "rswaf", (-1.0, 1.0), True, "all"),
    "softsign_iqf_quirk": ("softsign", "softsign", "iqf", (-1.0, 1.0), True, "all"),
    "softsign_iqf_exact": ("softsign", "softsign", "iqf", (-1.0, 1.0), False, "all"),
    "sigmoid_rbf_01": ("sigmoid", "sigmoid_fast", "rbf", (0.0, 1.0), True, "all"),
    "softsign_rbf_nobase": ("softsign", "softsign", "rbf", (-1.0, 1.0), True, "none"),
    "softsign_rbf_base0": ("softsign", "softsign", "rbf", (-1.0, 1.0), True, "first"),
    "identity_rbf_nobase": ("identity", "identity", "rbf", (-1.0, 1.0), True, "none"),   # single layers only
}
CORE = ["tanhfast_rbf", "tanh_rswaf", "softsign_iqf_quirk", "softsign_iqf_exact", "softsign_rbf_nobase"]
FULL = CORE + ["sigmoid_rbf_01", "softsign_rbf_base0"]


@dataclass(frozen=True)
class Row:
    group: str
    widths: tuple
    G: int
    batches: tuple
    f64: tuple           # the classes of the layers, base activation on
    f32: tuple
    f64_nobase: tuple = None   # ... without it, where they differ (P is smaller)
    f32_nobase: tuple = None


PAIR = (WIDE_IN, WIDE_OUT)
ROWS = [
    # pair, width sweep: tn = 256 / 252 / 250 / 256; (MV, MW) = (8, 2), (16, 4), (16, 4), (32, 8)
    Row("pair_width", (400, 1, 400), 5, (1, 9), PAIR, PAIR),
    Row("pair_width", (96, 7, 96), 5, (1, 9), PAIR, PAIR),
    Row("pair_width", (41, 10, 41), 5, (1, 9), PAIR, PAIR),
    Row("pair_width", (128, 16, 128), 5, (1, 9), PAIR, PAIR),
    # pair, grid sweep: G = 2 drops layer 0 of [41, 10, 41] to the column class; G = 32 has cw = 25
    Row("pair_grid", (41, 10, 41), 2, (1, 9), (COL, WIDE_OUT), (COL, WIDE_OUT)),
    Row("pair_grid", (128, 16, 128), 2, (1, 9), PAIR, PAIR),
    Row("pair_grid", (41, 10, 41), 32, (1, 9), PAIR, PAIR),
    Row("pair_grid", (128, 16, 128), 32, (1, 9), PAIR, PAIR),
    # pair, batch edges: kPairMaxK = 64 (two launches), 65 (the four-launch fallback)
    Row("pair_batch", (41, 10, 41), 5, (64, 65), PAIR, PAIR),
    # wide-out alone: one partial row chunk, 64 + 1, two chunks and a ragged one (kWOB = 64)
    Row("wideout", (3, 17), 5, (1, 9), (WIDE_OUT,), (WIDE_OUT,)),
    Row("wideout", (3, 65), 5, (1, 9), (WIDE_OUT,), (WIDE_OUT,)),
    Row("wideout", (3, 130), 5, (1, 9), (WIDE_OUT,), (WIDE_OUT,)),
    Row("wideout", (3, 17), 32, (1, 9), (WIDE_OUT,), (WIDE_OUT,)),
    Row("wideout", (3, 65), 32, (1, 9), (WIDE_OUT,), (WIDE_OUT,)),
    Row("wideout", (3, 130), 32, (1, 9), (WIDE_OUT,), (WIDE_OUT,)),
    # wide-in alone, n_in != n_out
    Row("widein", (400, 1), 5, (1, 9), (WIDE_IN,), (WIDE_IN,)),
    Row("widein", (64, 16), 5, (1, 9), (WIDE_IN,), (WIDE_IN,)),
    # mixed-class chains (the generic layer-by-layer branches of rhs_t / vjp_t)
    Row("mixed", (2, 40, 2), 5, (1, 9), (WIDE_OUT, COL), (WIDE_OUT, COL)),
    Row("mixed", (2, 64, 2), 5, (1, 9), (WIDE_OUT, WIDE_IN), (WIDE_OUT, COL)),
    Row("mixed", (20, 20, 20), 5, (1, 9), (WIDE_OUT, WIDE_OUT), (WIDE_OUT, WIDE_OUT)),
    Row("mixed", (48, 10, 10, 48), 5, (1, 9), (WIDE_IN, COL, WIDE_OUT), (WIDE_IN, COL, WIDE_OUT)),
    # class edges: P = 2040 / 2100 across the column / wide-in line; the one-launch chain kernel at kChainDim
    Row("edge", (34, 10, 34), 5, (1, 9), (COL, WIDE_OUT), (COL, WIDE_OUT)),
    Row("edge", (35, 10, 35), 5, (1, 9), PAIR, PAIR, (COL, WIDE_OUT), (COL, WIDE_OUT)),
    Row("edge", (16, 16, 16), 5, (1, 9), (COL, COL), (COL, COL)),
]

# the class tuples the matrix has to reach, per dtype (test_layer_cases_cpu.py: each claimed by a record)
REQUIRED = {
    "f64": [PAIR, (COL, WIDE_OUT), (WIDE_OUT,), (WIDE_IN,), (WIDE_OUT, COL), (WIDE_OUT, WIDE_IN),
            (WIDE_OUT, WIDE_OUT), (WIDE_IN, COL, WIDE_OUT), (COL, COL)],
    "f32": [PAIR, (COL, WIDE_OUT), (WIDE_OUT,), (WIDE_IN,), (WIDE_OUT, COL), (WIDE_OUT, WIDE_OUT),
            (WIDE_IN, COL, WIDE_OUT), (COL, COL)],
}
REQUIRED_INSTANTIATIONS = [(8, 2), (16, 4), (32, 8)]


@dataclass(frozen=True)
class Case:
    row: Row
    variant: str
    dtype: str      # "f64" / "f32"
    B: int

    @property
    def id(self):
        w = "x".join(str(v) for v in self.row.widths)
        return f"{self.row.group}-{w}-G{self.row.G}-{self.variant}-{self.dtype}-B{self.B}"

    @property
    def seed(self):
        return zlib.crc32(self.id.encode())

    @property
    def n_layers(self):
        return len(self.row.widths) - 1

    @property
    def base(self):
        mode = VARIANTS[self.variant][5]
        return [mode == "all" or (mode == "first" and l == 0) for l in range(self.n_layers)]

    @property
    def classes(self):
        """The classes this record is meant to reach (stated by hand in ROWS)."""
        r = self.row
        if not self.base[0] and getattr(r, self.dtype + "_nobase") is not None:
            return getattr(r, self.dtype + "_nobase")
        return getattr(r, self.dtype)

    @property
    def is_pair(self):
        return self.classes == PAIR

    def specs(self):
        n0, n1, basis, lims, quirk, _ = VARIANTS[self.variant]
        w, base = self.row.widths, self.base
        return [O.LayerSpec(w[l], w[l + 1], self.row.G, n0 if l == 0 else n1, basis, base[l], lims, None, quirk)
                for l in range(self.n_layers)]

    def np_dtype(self):
        return np.float64 if self.dtype == "f64" else np.float32

    def data(self):
        """(p, u, ȳ) in float64.  Glorot-uniform parameters (no W block without the base activation), inputs
        uniform inside the grid limits, ȳ standard normal; an fp32 record's values are rounded to fp32 first."""
        rng = np.random.default_rng(self.seed)
        parts = []
        for s in self.specs():
            lim = np.sqrt(6.0 / (s.out_dims + s.grid_len * s.in_dims))
            parts.append(rng.uniform(-lim, lim, s.out_dims * s.grid_len * s.in_dims))
            if s.use_base_act:
                lim = np.sqrt(6.0 / (s.out_dims + s.in_dims))
                parts.append(rng.uniform(-lim, lim, s.out_dims * s.in_dims))
        lo, hi = VARIANTS[self.variant][3]
        p = np.concatenate(parts)
        u = rng.uniform(lo, hi, (self.B, self.row.widths[0]))
        yb = rng.normal(size=(self.B, self.row.widths[-1]))
        dt = self.np_dtype()
        return tuple(a.astype(dt).astype(np.float64) for a in (p, u, yb))


def _cases():
    out = []
    for r in ROWS:
        for B in r.batches:
            names = list(FULL if B != 1 else CORE)     # every row keeps the first four variants and no-base
            if len(r.widths) == 2:
                names.append("identity_rbf_nobase")
            for v in names:
                for dt in ("f64", "f32"):
                    out.append(Case(r, v, dt, B))
    return out


CASES = _cases()


def np_layers(specs):
    return [N.Layer(s.in_dims, s.out_dims, s.grid_len, s.normalizer, s.basis, s.use_base_act, s.grid_lims,
                    s.denominator, s.iqf_reference_quirk) for s in specs]


# ---- the error scale ------------------------------------------------------------------------------------------
def _norm_parts(name, x, dx):
    """(n, n_err, n'_s): the normalised input, its error scale and the scale of the Ω-form derivative."""
    n = N.NORMS[name](x)
    d1 = np.abs(N.dnorm(name, x, n))
    n_err = np.abs(n) + d1 * dx
    if name in ("tanh", "tanh_fast"):
        dn_s = 1 + n * n + 2 * np.abs(n) * n_err                     # 1 - Ω²
    elif name == "softsign":
        a = 1 - np.abs(n)
        dn_s = a * a + 2 * np.abs(a) * (1 + n_err)                   # (1 - |Ω|)²
    elif name in ("sigmoid", "sigmoid_fast"):
        dn_s = np.abs(n * (1 - n)) + np.abs(n) + np.abs(1 - 2 * n) * n_err   # Ω(1 - Ω)
    else:
        dn_s = np.ones_like(x)
    return n, n_err, dn_s


def _basis_parts(L, a, a_err):
    """(φ_s, ψ_s) at the basis argument a (K, I, G) with error scale a_err."""
    a2 = a * a
    if L.basis == "rbf":
        phi = np.exp(-a2)
        phi_t, dphi = phi, 2 * np.abs(a) * phi
        psi_t, dpsi = 2 * np.abs(a) * phi, (2 + 4 * a2) * phi
    elif L.basis == "rswaf":
        t = np.tanh(a)
        phi = 1 - t * t
        phi_t, dphi = 1 + t * t, 2 * np.abs(t) * phi
        psi_t, dpsi = 2 * np.abs(t) * (1 + t * t), 2 * phi * phi + 4 * t * t * phi
    else:
        phi = 1 / (1 + a2)
        phi_t, dphi = phi, 2 * np.abs(a) * phi * phi
        if L.iqf_reference_quirk:
            psi_t, dpsi = 2 * np.abs(a) * phi, 2 * phi + 4 * a2 * phi * phi
        else:
            psi_t, dpsi = 2 * np.abs(a) * phi * phi, 2 * phi * phi + 8 * a2 * phi ** 3
    return phi_t + dphi * a_err, psi_t + dpsi * a_err


def _layer_parts(L, x, dx):
    n, n_err, dn_s = _norm_parts(L.normalizer, x, dx)
    invh = float(L.invh)
    knot = L.grid.astype(np.float64)[None, None, :]
    a = (n[:, :, None] - knot) * invh
    a_err = invh * (n_err[:, :, None] + np.abs(knot))
    phi_s, psi_s = _basis_parts(L, a, a_err)
    s = N.sigmoid(x)
    sw = x * s
    d1 = s + x * s * (1 - s)
    d2 = s * (1 - s) * (2 + x * (1 - 2 * s))
    sw_s = np.abs(sw) + np.abs(d1) * dx
    dsw_s = np.abs(sw) + s * (1 + np.abs(sw)) + np.abs(d2) * dx
    return phi_s, psi_s, dn_s, sw_s, dsw_s, invh


def _abs_split(L, p):
    C, W = L.split(np.abs(p))
    return C, W


def _fwd_scale(L, p, x, dx):
    phi_s, _, _, sw_s, _, _ = _layer_parts(L, x, dx)
    C, W = _abs_split(L, p)
    y = phi_s.reshape(x.shape[0], L.I * L.G) @ C.T
    if L.use_base_act:
        y = y + sw_s @ W.T
    return y


def _vjp_scale(L, p, x, dx, yb_s):
    phi_s, psi_s, dn_s, sw_s, dsw_s, invh = _layer_parts(L, x, dx)
    C, W = _abs_split(L, p)
    K = x.shape[0]
    Cbar = yb_s.T @ phi_s.reshape(K, L.I * L.G)
    bb = (yb_s @ C).reshape(K, L.I, L.G)
    xb = (psi_s * bb).sum(axis=2) * invh * dn_s
    parts = [Cbar.T.reshape(-1)]
    if L.use_base_act:
        xb = xb + (yb_s @ W) * dsw_s
        parts.append((yb_s.T @ sw_s).T.reshape(-1))
    return xb, np.concatenate(parts)


def _vjp_mag(L, p, x, dg):
    """|J|ᵀ·dg and |∂p̄/∂ȳ|·dg with the plain magnitudes: how an error scale dg of the cotangent reaches x̄ and p̄."""
    n = N.NORMS[L.normalizer](x)
    invh = float(L.invh)
    a = (n[:, :, None] - L.grid.astype(np.float64)[None, None, :]) * invh
    if L.basis == "rbf":
        phi = np.exp(-a * a)
        psi = 2 * np.abs(a) * phi
    elif L.basis == "rswaf":
        t = np.tanh(a)
        phi = 1 - t * t
        psi = 2 * np.abs(t) * phi
    else:
        phi = 1 / (1 + a * a)
        psi = 2 * np.abs(a) * phi * (1 if L.iqf_reference_quirk else phi)
    C, W = _abs_split(L, p)
    K = x.shape[0]
    xb = (psi * (dg @ C).reshape(K, L.I, L.G)).sum(axis=2) * invh * np.abs(N.dnorm(L.normalizer, x, n))
    parts = [(dg.T @ phi.reshape(K, L.I * L.G)).T.reshape(-1)]
    if L.use_base_act:
        xb = xb + (dg @ W) * np.abs(N.dswish(x))
        parts.append((dg.T @ np.abs(N.swish(x))).T.reshape(-1))
    return xb, np.concatenate(parts)


_EPS = 1e-7


def _vjp_first_order(L, p, x, dx, g, dg):
    """x̄ and p̄ scales of one layer of a chain: the single-layer scale at (x, |g|), the part of it linear in dx,
    and dg through the plain magnitudes."""
    xb, pb = _vjp_scale(L, p, x, np.zeros_like(x), np.abs(g))
    if np.any(dx):
        xb1, pb1 = _vjp_scale(L, p, x, _EPS * dx, np.abs(g))
        xb = xb + np.maximum(xb1 - xb, 0) / _EPS
        pb = pb + np.maximum(pb1 - pb, 0) / _EPS
    if np.any(dg):
        xm, pm = _vjp_mag(L, p, x, dg)
        xb, pb = xb + xm, pb + pm
    return xb, pb


def _floor(s):
    return s + 1e-3 * np.max(s)


def layer_error_scale(spec, p, x, ybar):
    """(y, x̄, p̄) scales of one layer at exact inputs (the single-layer entry points)."""
    L = np_layers([spec])[0]
    x = np.asarray(x, np.float64)
    zero = np.zeros_like(x)
    xb, pb = _vjp_scale(L, p, x, zero, np.abs(np.asarray(ybar, np.float64)))
    return _floor(_fwd_scale(L, p, x, zero)), _floor(xb), _floor(pb)


def chain_error_scale(specs, p, u, ybar, hidden_exact=False):
    """(y, x̄, p̄) scales of a chain against the oracle: the hidden layers' forward error enters the later layers' y,
    x̄ and p̄, the later layers' x̄ error the earlier layers' x̄ and p̄, to first order (module docstring).
    hidden_exact: the hidden values are taken as exact (composition_error_scale)."""
    Ls = np_layers(specs)
    p, u, ybar = (np.asarray(a, np.float64) for a in (p, u, ybar))
    offs = np.cumsum([0] + [l.P for l in Ls])
    xs, dxs = [u], [np.zeros_like(u)]
    for l, L in enumerate(Ls):
        pl = p[offs[l]:offs[l + 1]]
        y_s = _fwd_scale(L, pl, xs[-1], dxs[-1])
        xs.append(L.fwd(pl, xs[-1]))
        dxs.append(np.zeros_like(y_s) if hidden_exact and l < len(Ls) - 1 else y_s)
    g, dg = ybar, np.zeros_like(ybar)
    pb_parts = [None] * len(Ls)
    for l in range(len(Ls) - 1, -1, -1):
        pl = p[offs[l]:offs[l + 1]]
        xb_s, pb_s = _vjp_first_order(Ls[l], pl, xs[l], dxs[l], g, dg)
        pb_parts[l] = _floor(pb_s)
        g, _ = Ls[l].vjp(pl, xs[l], g)
        dg = xb_s
    return _floor(dxs[-1]), _floor(dg), np.concatenate(pb_parts)


def composition_error_scale(specs, p, u, ybar):
    """(y, x̄, p̄) scales of a chain result against the composition of the single-layer calls on the same device,
    when both see the same hidden values bit for bit (the surrogate pair's forward equals the layer calls bitwise):
    every layer's single-layer scale at exact inputs, and the rounding of each hidden cotangent carried down once
    through the plain |J|ᵀ of the layers below."""
    return chain_error_scale(specs, p, u, ybar, hidden_exact=True)


def error_scale(case):
    p, u, yb = case.data()
    return chain_error_scale(case.specs(), p, u, yb)


# ---- wrong restatements (test_layer_cases_cpu.py: the bound has to tell them from the oracle) -------------------
class _MutLayer(N.Layer):
    """kanode_np.Layer with one thing wrong: drop_knot (that knot's coefficient row is never read), no_base_last
    (the base term of the last input is omitted), flip_quirk (the iqf pullback of the other setting), f32_knots
    (knots accumulated with a Float32 step)."""

    def __init__(self, spec, drop_knot=None, no_base_last=False, flip_quirk=False, f32_knots=False):
        q = spec.iqf_reference_quirk
        super().__init__(spec.in_dims, spec.out_dims, spec.grid_len, spec.normalizer, spec.basis, spec.use_base_act,
                         spec.grid_lims, None, (not q) if flip_quirk else q)
        self.drop_knot, self.no_base_last = drop_knot, no_base_last and spec.use_base_act
        if f32_knots:
            lo, hi = np.float32(spec.grid_lims[0]), np.float32(spec.grid_lims[1])
            h = np.float32((hi - lo) / np.float32(self.G - 1))
            self.grid = np.array([lo + np.float32(j) * h for j in range(self.G)], np.float32)

    def split(self, p):
        C, W = super().split(p)
        if self.drop_knot is not None:
            C = C.copy()
            C.reshape(self.O, self.I, self.G)[:, :, self.drop_knot] = 0
        if self.no_base_last:
            W = W.copy()
            W[:, self.I - 1] = 0
        return C, W

    def vjp(self, p, x, ybar):
        xbar, pbar = super().vjp(p, x, ybar)
        if self.drop_knot is not None or self.no_base_last:
            pbar = pbar.copy()
            nC = self.O * self.G * self.I
            if self.drop_knot is not None:
                pbar[:nC].reshape(self.I, self.G, self.O)[:, self.drop_knot, :] = 0
            if self.no_base_last:
                pbar[nC:].reshape(self.I, self.O)[self.I - 1, :] = 0
        return xbar, pbar


class _Tile0Layer(N.Layer):
    """The output rows o >= 64 (and their parameter cotangents) computed from column tile 0's basis: column k reads
    the layer input of column k mod 8."""

    def __init__(self, spec):
        super().__init__(spec.in_dims, spec.out_dims, spec.grid_len, spec.normalizer, spec.basis, spec.use_base_act,
                         spec.grid_lims, None, spec.iqf_reference_quirk)

    def fwd(self, p, x):
        y = super().fwd(p, x)
        y[:, 64:] = super().fwd(p, x[np.arange(x.shape[0]) % 8])[:, 64:]
        return y

    def vjp(self, p, x, ybar):
        xbar, pbar = super().vjp(p, x, ybar)
        _, pb0 = super().vjp(p, x[np.arange(x.shape[0]) % 8], ybar)
        nC = self.O * self.G * self.I
        pbar[:nC].reshape(-1, self.O)[:, 64:] = pb0[:nC].reshape(-1, self.O)[:, 64:]
        if self.use_base_act:
            pbar[nC:].reshape(-1, self.O)[:, 64:] = pb0[nC:].reshape(-1, self.O)[:, 64:]
        return xbar, pbar


def mutated_chain(case, which, knot=None):
    """The numpy chain of `case` with one wrong restatement: "drop_knot" (knot row `knot` of the last layer: an
    index, a list, "alternate", default the last), "flip_quirk" (every layer), "no_base_last" (the last layer that has a base term), "f32_knots"
    (every layer), "tile0" (the last layer)."""
    specs = case.specs()
    last = len(specs) - 1
    layers = []
    based = [l for l, s in enumerate(specs) if s.use_base_act]
    for l, s in enumerate(specs):
        if which == "drop_knot" and l == last:
            if knot == "alternate":          # every other knot row, counted from the last
                knot = list(range(s.grid_len - 1, -1, -2))
            layers.append(_MutLayer(s, drop_knot=s.grid_len - 1 if knot is None else knot))
        elif which == "flip_quirk":
            layers.append(_MutLayer(s, flip_quirk=True))
        elif which == "no_base_last" and based and l == based[-1]:
            layers.append(_MutLayer(s, no_base_last=True))
        elif which == "f32_knots":
            layers.append(_MutLayer(s, f32_knots=True))
        elif which == "tile0" and l == last:
            layers.append(_Tile0Layer(s))
        else:
            layers.append(_MutLayer(s))
    return N.Chain(layers)
