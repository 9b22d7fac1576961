"""The parity matrix's case table and error scale, checked on the CPU (tests/layer_cases.py; numpy and the C oracle
only, no kernel): the records reach the kernel classes they claim, the scale is sound (the fp32 oracle and the
differently-ordered numpy restatement stay inside it on every record) and it discriminates (wrong restatements of
the layer leave it), and the oracle is pinned with mpmath for the rswaf and exact-iqf bases.

Measured here (worst err/bound per group, y / x̄ / p̄):
  fp32 C oracle against fp64 C oracle, RTOL 5e-6:  pair_width 0.008 / 5e-5 / 0.010, pair_grid 0.007 / 8e-4 / 0.023,
    pair_batch 0.002 / 7e-5 / 0.005, wideout 0.021 / 0.003 / 0.034, widein 0.008 / 0.008 / 0.035,
    mixed 0.006 / 2e-4 / 0.018, edge 0.002 / 5e-5 / 0.017
  numpy against C oracle in fp64, RTOL 1e-13: at most 0.002 / 9e-4 / 0.006
The single layers use a tenth of the bound at most; the chain x̄ figures of 1e-4 and less are not accuracy but the
worst-case compounding of the chain scale (below).
Each wrong restatement has to leave the bound on y, x̄ or p̄ of the record itself, under the chain scale
(test_discrimination); the comparisons of single layers are asserted on their own (test_discrimination_per_layer).
Least chain-level err/bound over the records: knot row 2.4, iqf quirk 3.0, base term 68, Float32-step knots 2.4e4,
tile-0 basis 316.  Two narrowings, for reasons that do not depend on this scale:
  * the last knot's row at G = 32 with rbf / rswaf: every normalised input lies at least 0.24·invh = 3.7 knot widths
    below the last knot (|n| <= tanh 1 = 0.76, softsign <= 0.5, sigmoid <= 0.74), so the dropped terms are below
    e^-13.8 of the sum.  43 of those 92 records still see the single row and are asserted on it; only the 49 where
    it is measurably unseen (err/bound <= 1, down to 2e-12; a single-sample record may have no input near any one
    knot at all) drop every other knot row, counted from the last, instead.
  * Float32-step knots in fp32 records: the knots move by a few fp32 ulps, which is the size of the rounding of
    n - knot that the fp32 evaluation itself commits (measured err/bound 0.01 .. 0.15).  They are asked of the fp64
    records of the same shapes.
What the chain scale against the oracle cannot see: it carries every hidden layer's worst-case error through the next
layer's |J|, and in fp32 that exceeds the size of x̄ on most multi-layer records (test_chain_level_error_of_xbar
counts them: an x̄ of all zeros stays inside it on 16 of the 388 multi-layer records, a 1 % error on 150).  The discriminating chain check is the comparison with the layer composition on the same device
under composition_error_scale: there x̄ = 0 and p̄ = 0 of layer 0 leave the bound on every multi-layer record (by
>= 5x) and a 1 % error on all but 23 fp32 ones."""
import functools

import mpmath as mp
import numpy as np
import pytest
import torch

import layer_cases as LC
from gpu_util import RTOL, assert_close
from oracle import kanode_np as N
from oracle import oracle as O

BY_ID = {c.id: c for c in LC.CASES}
TDT = {"f64": torch.float64, "f32": torch.float32}


def _ratio(got, ref, scale, rtol):
    return float(np.max(np.abs(np.asarray(got, np.float64) - ref) / (rtol * scale)))


@functools.lru_cache(maxsize=None)
def _ref(cid):
    """(p, u, ȳ, specs, (y, x̄, p̄) of the fp64 C oracle, the three scales): computed once per record."""
    c = BY_ID[cid]
    p, u, yb = c.data()
    specs = c.specs()
    y = O.chain_fwd(specs, p, u)
    xb, pb = O.chain_vjp(specs, p, u, yb)
    out = (p, u, yb, specs, (y, xb, pb), LC.error_scale(c))
    for a in (p, u, yb, y, xb, pb) + out[5]:
        a.setflags(write=False)
    return out


def test_table_is_complete():
    assert len(BY_ID) == len(LC.CASES)            # ids are unique
    rows = {(r.widths, r.G, r.batches) for r in LC.ROWS}
    for r in LC.ROWS:
        for B in r.batches:
            for dt in ("f64", "f32"):
                have = {c.variant for c in LC.CASES if c.row is r and c.B == B and c.dtype == dt}
                assert set(LC.CORE) <= have, (r, B, dt)
    assert len(rows) == len(LC.ROWS)


@pytest.mark.parametrize("cid", list(BY_ID))
def test_record_reaches_its_classes(cid):
    c = BY_ID[cid]
    esize = 8 if c.dtype == "f64" else 4
    got = tuple(LC.kernel_class(s.in_dims, s.out_dims, s.grid_len, s.use_base_act, esize) for s in c.specs())
    assert got == c.classes


@pytest.mark.parametrize("dt", ["f64", "f32"])
def test_every_class_pair_and_load_slot_choice_is_claimed(dt):
    claimed = {c.classes for c in LC.CASES if c.dtype == dt}
    for need in LC.REQUIRED[dt]:
        assert need in claimed, need
    # the fp32 column kernel with I = 64 ([2, 64, 2], where fp64 takes the wide-in kernel)
    assert any(c.dtype == "f32" and c.row.widths == (2, 64, 2) and c.classes[1] == LC.COL for c in LC.CASES)
    inst = set()
    for c in LC.CASES:
        if c.dtype == dt:
            for s, k in zip(c.specs(), c.classes):
                if k == LC.WIDE_IN:
                    inst.add(LC.widein_instantiation(s.in_dims, s.out_dims, s.grid_len))
    assert inst == set(LC.REQUIRED_INSTANTIATIONS)
    # the widths of the sweep: tn = 256 / 252 / 250 / 256, and cw = 25 at G = 32
    assert [LC.widein_slots(I, O_, 5)[0] for I, O_ in ((400, 1), (96, 7), (41, 10), (128, 16))] == [256, 252, 250, 256]
    assert LC.widein_slots(41, 10, 32)[1] == 25


@pytest.mark.parametrize("cid", list(BY_ID))
def test_scale_is_sound(cid):
    """No record is excused: the fp32 C oracle (fp32 records) and the numpy restatement, which sums in another
    order (every record), against the fp64 C oracle."""
    c = BY_ID[cid]
    p, u, yb, specs, (y, xb, pb), (ys, xs, ps) = _ref(cid)
    ch = N.Chain(LC.np_layers(specs))
    xn, pn = ch.vjp(p, u, yb)
    assert_close(ch.fwd(p, u), y, ys, RTOL[torch.float64], "numpy y")
    assert_close(xn, xb, xs, RTOL[torch.float64], "numpy xbar")
    assert_close(pn, pb, ps, RTOL[torch.float64], "numpy pbar")
    if c.dtype == "f32":
        f = np.float32
        assert np.array_equal(p.astype(f), p) and np.array_equal(u.astype(f), u) and np.array_equal(yb.astype(f), yb)
        y32 = O.chain_fwd(specs, p.astype(f), u.astype(f))
        xb32, pb32 = O.chain_vjp(specs, p.astype(f), u.astype(f), yb.astype(f))
        assert y32.dtype == f
        assert_close(y32, y, ys, RTOL[torch.float32], "fp32 oracle y")
        assert_close(xb32, xb, xs, RTOL[torch.float32], "fp32 oracle xbar")
        assert_close(pb32, pb, ps, RTOL[torch.float32], "fp32 oracle pbar")


def _light_tails(c):
    return c.row.G == 32 and VARIANT_BASIS[c.variant] in ("rbf", "rswaf")


VARIANT_BASIS = {k: v[2] for k, v in LC.VARIANTS.items()}
MUTATIONS = {
    # name: (the records of its group, why the others are left out)
    "drop_knot": lambda c: True,
    "flip_quirk": lambda c: VARIANT_BASIS[c.variant] == "iqf",
    "no_base_last": lambda c: any(c.base),
    "f32_knots": lambda c: c.row.G == 32 and c.dtype == "f64",     # (fp32 records: see the module docstring)
    "tile0": lambda c: c.B == 9 and c.row.widths[-1] > 64,
}


def _chain_ratio(c, which, knot=None):
    """The largest err/bound of the wrong restatement on y, x̄, p̄ of the record under the chain scale."""
    p, u, yb, specs, (y, xb, pb), (ys, xs, ps) = _ref(c.id)
    rtol = RTOL[TDT[c.dtype]]
    ch = LC.mutated_chain(c, which, knot)
    xn, pn = ch.vjp(p, u, yb)
    return max(_ratio(ch.fwd(p, u), y, ys, rtol), _ratio(xn, xb, xs, rtol), _ratio(pn, pb, ps, rtol))


def _layer_ratio(c, which, knot=None):
    """... and over every layer alone, at the oracle's hidden inputs and cotangents, under the single-layer scale
    (the GPU matrix compares layer_forward / layer_vjp that way)."""
    p, u, yb, specs, _, _ = _ref(c.id)
    rtol = RTOL[TDT[c.dtype]]
    ch = LC.mutated_chain(c, which, knot)
    offs = np.cumsum([0] + [s.param_length() for s in specs])
    xs_l = [u]
    for l, s in enumerate(specs[:-1]):
        xs_l.append(O.layer_fwd(s, p[offs[l]:offs[l + 1]], xs_l[-1]))
    g, worst = yb, 0.0
    for l in range(len(specs) - 1, -1, -1):
        pl = p[offs[l]:offs[l + 1]]
        ry = O.layer_fwd(specs[l], pl, xs_l[l])
        rxb, rpb = O.layer_vjp(specs[l], pl, xs_l[l], g)
        sy, sx, sp = LC.layer_error_scale(specs[l], pl, xs_l[l], g)
        mxb, mpb = ch.layers[l].vjp(pl, xs_l[l], g)
        worst = max(worst, _ratio(ch.layers[l].fwd(pl, xs_l[l]), ry, sy, rtol), _ratio(mxb, rxb, sx, rtol),
                    _ratio(mpb, rpb, sp, rtol))
        g = rxb
    return worst


def _missed(which, ratio):
    """The records of the mutation's group that `ratio` does not tell from the oracle.  Dropped knot row: the last
    one; a G = 32 rbf / rswaf record where that single row is measurably unseen (module docstring) drops every other
    row instead."""
    group = [c for c in LC.CASES if MUTATIONS[which](c)]
    assert len(group) >= 60
    missed, narrowed = {}, 0
    for c in group:
        r = ratio(c, which)
        if not r > 1.0 and which == "drop_knot" and _light_tails(c):
            narrowed += 1
            r = ratio(c, which, "alternate")
        if not r > 1.0:
            missed[c.id] = r
    return missed, narrowed, len(group)


@pytest.mark.parametrize("which", list(MUTATIONS))
def test_discrimination(which):
    """Every wrong restatement leaves the chain's bound (err/bound > 1 on y, x̄ or p̄) in every record of its group."""
    missed, narrowed, n = _missed(which, _chain_ratio)
    assert not missed, f"{which}: not told from the oracle in {len(missed)} of {n} records: {missed}"
    assert narrowed <= 49      # the records counted in the module docstring, not more


@pytest.mark.parametrize("which", list(MUTATIONS))
def test_discrimination_per_layer(which):
    """... and, separately, the bound of some single layer's comparison."""
    missed, _, n = _missed(which, _layer_ratio)
    assert not missed, f"{which}: not told from the oracle layer by layer in {len(missed)} of {n} records: {missed}"


CHAIN_BLIND_ZERO, CHAIN_BLIND_1PCT, COMPOSITION_BLIND_1PCT = 16, 150, 23    # of 388 multi-layer records, as measured


def test_chain_level_error_of_xbar():
    """A wrong x̄ (all zeros, or off by 1 %) and a wrong p̄ of layer 0, as a chain-level fault that every layer call
    alone would not show (a fused pullback that loses the hidden cotangent), in the chain comparisons of every
    multi-layer record.  Against the layer composition (composition_error_scale) zeros leave the bound on every
    record, and 1 % on every fp64 record by >= 1e3x and on all but 23 fp32 ones (rswaf, whose 1 + tanh² terms are
    large, and G = 32, where 5e-6·invh·2 of Σ|terms| is itself near 1 % of x̄).  Against the oracle (the worst-case
    chain scale) zeros stay inside the bound on 16 fp32 records and 1 % on 150: the counts are pinned, so that the
    looseness stays visible and a change that worsens it fails."""
    blind_zero = blind_1pct = comp_1pct = 0
    multi = [c for c in LC.CASES if c.n_layers > 1]
    for c in multi:
        p, u, yb, specs, (y, xb, pb), (ys, xs, ps) = _ref(c.id)
        rtol = RTOL[TDT[c.dtype]]
        _, xc, pc = LC.composition_error_scale(specs, p, u, yb)
        P0 = specs[0].param_length()
        zero_x = _ratio(np.zeros_like(xb), xb, xc, rtol)
        zero_p = _ratio(np.zeros(P0), pb[:P0], pc[:P0], rtol)
        assert zero_x > 1 and zero_p > 1, (c.id, zero_x, zero_p)
        comp_1pct += not (0.01 * zero_x > 1 and 0.01 * zero_p > 1)
        if c.dtype == "f64":
            assert 0.01 * zero_x > 1e3 and 0.01 * zero_p > 1e3, (c.id, zero_x, zero_p)
        z = _ratio(np.zeros_like(xb), xb, xs, rtol)
        blind_zero += not z > 1
        blind_1pct += not 0.01 * z > 1
    assert len(multi) == 388
    assert blind_zero <= CHAIN_BLIND_ZERO and blind_1pct <= CHAIN_BLIND_1PCT and comp_1pct <= COMPOSITION_BLIND_1PCT, \
        (blind_zero, blind_1pct, comp_1pct)


def _mp_single_layer(spec, p, x, yb, outs, pbs):
    """y[o] for o in outs and p̄[j] for j in pbs of one KDense layer at one sample, 40 digits (tanh / softsign
    normalizer; rswaf / exact iqf basis)."""
    mp.mp.dps = 40
    G, I, Ox = spec.grid_len, spec.in_dims, spec.out_dims
    grid = [mp.mpf(float(v)) for v in N.knots(G)]
    invh = mp.mpf(float(N.inv_h(N.default_denominator(G))))
    nC = Ox * G * I

    def phi(i, g):
        xv = mp.mpf(float(x[i]))
        n = mp.tanh(xv) if spec.normalizer == "tanh" else xv / (1 + abs(xv))
        a = (n - grid[g]) * invh
        return 1 - mp.tanh(a) ** 2 if spec.basis == "rswaf" else 1 / (1 + a * a)

    def swish(i):
        xv = mp.mpf(float(x[i]))
        return xv / (1 + mp.exp(-xv))

    ys = []
    for o in outs:
        s = mp.mpf(0)
        for i in range(I):
            for g in range(G):
                s += mp.mpf(float(p[o + Ox * (g + G * i)])) * phi(i, g)
            s += mp.mpf(float(p[nC + o + Ox * i])) * swish(i)
        ys.append(s)
    ps = []
    for j in pbs:
        if j < nC:
            o, c = j % Ox, j // Ox
            ps.append(mp.mpf(float(yb[o])) * phi(c // G, c % G))
        else:
            o, i = (j - nC) % Ox, (j - nC) // Ox
            ps.append(mp.mpf(float(yb[o])) * swish(i))
    return ys, ps


@pytest.mark.parametrize("cid", ["wideout-3x17-G5-tanh_rswaf-f64-B1", "widein-64x16-G5-softsign_iqf_exact-f64-B1"])
def test_oracle_vs_mpmath_rswaf_and_exact_iqf(cid):
    p, u, yb, specs, (y, xb, pb), (ys, xs, ps) = _ref(cid)
    spec = specs[0]
    assert spec.basis in ("rswaf", "iqf") and not (spec.basis == "iqf" and spec.iqf_reference_quirk)
    Ox, nC = spec.out_dims, spec.out_dims * spec.grid_len * spec.in_dims
    outs = [0, 1, Ox // 2, Ox - 1]
    pbs = [0, nC // 2 + 1, nC - 1, nC + Ox * spec.in_dims - 1]
    my, mpb = _mp_single_layer(spec, p, u[0], yb[0], outs, pbs)
    rtol = RTOL[torch.float64]
    for o, v in zip(outs, my):
        assert abs(float(v - mp.mpf(float(y[0, o])))) <= rtol * ys[0, o]
    for j, v in zip(pbs, mpb):
        assert abs(float(v - mp.mpf(float(pb[j])))) <= rtol * ps[j]
