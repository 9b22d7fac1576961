"""The case table and the bar of the Fisher-KPP per-point parity matrix, checked on the CPU (tests/fk_cases.py; numpy
and the C oracle only, no kernel): the records reach the instantiations and launch classes they claim, the scale is
sound (the fp32 C oracle and a numpy fp32 restatement of the recurrence stay inside it on every fp32 record, the
float64 numpy model on every record) and it discriminates (seven wrong restatements of the kernels leave it).

Measured here, worst err/bound (du / λᵀJ / dp) against the fp64 C oracle:
  numpy float64 model, RTOL 1e-13, every record:                       0.002 / 0.002 / 0.040
  fp32 C oracle + numpy fp32 Laplacian, RTOL 5e-6, fp32 records:       direct 0.037 / 0.032 / 0.13, rec 0.032 / 0.029 /
    0.15, rec_corr 0.019 / 0.015 / 0.12 (dp: one serial fp32 sum per trajectory, up to 514 points)
  numpy fp32 recurrence (rec_anchor, Horner sweeps), fp32 REC records: 0.044 / 0.029 / 0.055, REC_CORR 0.029 / 0.024 /
    0.074
So layer_cases.layer_error_scale plus the Laplacian's Σ|terms| holds the recurrence in fp32 as it stands (its
a_err = invh·(|n| + |knot|) already covers the rounding of 2·z0·δ·j); no recurrence term was added.  The bounds
asserted below leave a factor 3 to 4 over these figures.

Each wrong restatement leaves the bound on du, λᵀJ or dp of every record of its group; no group had to be narrowed.
Least err/bound: last neighbour not wrapped 694 (484 records: nx >= 3, D != 0), nx = 1, 2 as a generic row 1.1e4
(184), float64-exact knots 1.4e4 (205 fp64 REC_CORR records), base term missing on a pair's second point 71 (584),
dW left at slot GL 1.0e3 (1130), points with q >= tpt skipped 4.1e3 (114 long records), first trip of the b-loop only
2.8e4 (12 grid-stride records)."""
import functools

import numpy as np
import pytest
import torch

import fk_cases as FC
from gpu_util import RTOL, assert_close

BY_ID = {c.id: c for c in FC.CASES}
TDT = {"f64": torch.float64, "f32": torch.float32}


def _ratio(got, ref, scale, rtol):
    return float(np.max(np.abs(np.asarray(got, np.float64) - ref) / (rtol * scale)))


def _ref(cid):
    """(p, u, λ, (du, λᵀJ, dp) of the fp64 C oracle, the three scales, the numpy layer at the points), read-only.  The
    twelve grid-stride records (10^6 points each) are computed once; the small ones are cheap and only pass through."""
    return (_ref_big if BY_ID[cid].grid_stride else _ref_small)(cid)


def _make_ref(cid):
    c = BY_ID[cid]
    p, u, lam = c.data()
    out = (p, u, lam, FC.oracle(c, p, u, lam), FC.fk_error_scale(c, p, u, lam), FC.np_base(c, p, u, lam))
    for a in (p, u, lam) + out[3] + out[4] + out[5]:
        a.setflags(write=False)
    return out


_ref_big = functools.lru_cache(maxsize=None)(_make_ref)
_ref_small = functools.lru_cache(maxsize=64)(_make_ref)


def test_table_is_complete():
    assert len(BY_ID) == len(FC.CASES) == 1322           # ids are unique; the count DESIGN §5 states
    for dt in ("f64", "f32"):
        for diff in ("D0", "Ddx2"):                      # every shape and variant exists at both
            a = {(c.variant, c.nx, c.B) for c in FC.CASES if c.dtype == dt and c.diff == diff}
            every = {(c.variant, c.nx, c.B) for c in FC.CASES if c.dtype == dt and c.diff in ("D0", "Ddx2")}
            assert a == every
        have = {(c.variant, c.nx, c.B) for c in FC.CASES if c.dtype == dt}
        for v in FC.VARIANTS:
            for nx in FC.SMALL_NX:
                assert (v, nx, 1) in have and (v, nx, 5) in have
        assert any(c.diff == "Dneg" and c.D_dx[0] < 0 for c in FC.CASES if c.dtype == dt)
        assert sum(c.diff == "Dref" for c in FC.CASES if c.dtype == dt) >= 4
    assert set(FC.SHAPES) == set(FC.SMALL_NX) | set(FC.EDGE_NX) == {1, 2, 3, 4, 5, 26, 255, 257, 512, 514}


@pytest.mark.parametrize("cid", list(BY_ID))
def test_record_reaches_its_classes(cid):
    """The hand-stated path, instantiation and launch class against the restated rules; the planted points."""
    c = BY_ID[cid]
    spec = c.spec()
    assert FC.fk_path(c.dtype, spec) == c.path
    assert FC.fk_instantiation(c.dtype, spec) == c.instantiation
    assert FC.fk_launch_class(c.nx) == c.launch
    assert FC.fk_grid_stride(c.nx, c.B) == (c.grid_stride, c.grid_stride)
    _, u, _ = c.data()
    if u.size >= 4:
        assert 0.0 in u and 1e4 in u and -1e4 in u
    if spec.normalizer == "identity" and u.size >= 5:
        assert 7.0 in u
    if c.dtype == "f32":
        assert np.array_equal(u.astype(np.float32), u)


@pytest.mark.parametrize("dt", ["f64", "f32"])
def test_required_is_covered(dt):
    claimed = set().union(*[c.claims for c in FC.CASES if c.dtype == dt])
    assert FC.REQUIRED[dt] <= claimed, FC.REQUIRED[dt] - claimed
    assert len([r for r in FC.REQUIRED[dt] if r[0] == "inst"]) == (6 if dt == "f64" else 5)
    # fp32 cannot reach softsign·REC_CORR·10: G = 10 is DIRECT there and runs the runtime-G kernel
    if dt == "f32":
        assert ("inst", "softsign", FC.REC_CORR, 10) not in claimed
        assert FC.fk_instantiation("f32", BY_ID["softsign_rbf_G10-f32-nx26-B5-Ddx2"].spec()) == ("runtime", FC.DIRECT, 0)
    # the long and the grid-stride classes carry one variant of each PATH
    for pred in (lambda c: c.launch[1] == "long", lambda c: c.grid_stride):
        assert {c.path for c in FC.CASES if c.dtype == dt and pred(c)} == {FC.DIRECT, FC.REC, FC.REC_CORR}
    # δ != 1, and the fp32 REC_CORR grid lengths below the fp32 limit
    assert FC.layer_consts(BY_ID["softsign_rbf_den_G5-f64-nx5-B1-D0"].spec()).delta == 1.25
    assert FC.layer_consts(BY_ID["sigmoid_rbf_01_G5-f64-nx5-B1-D0"].spec()).delta == 0.5


# worst err/bound asserted per group (du, λᵀJ, dp): the measured figures of the module docstring with headroom
SOUND = {
    "numpy": (0.01, 0.01, 0.12),
    ("c32", FC.DIRECT): (0.12, 0.1, 0.5), ("c32", FC.REC): (0.1, 0.1, 0.5), ("c32", FC.REC_CORR): (0.08, 0.06, 0.4),
    ("rec32", FC.REC): (0.15, 0.1, 0.2), ("rec32", FC.REC_CORR): (0.1, 0.08, 0.25),
}


@pytest.mark.parametrize("cid", list(BY_ID))
def test_scale_is_sound(cid):
    """No record is excused: the float64 numpy model (every record), the fp32 C oracle (every fp32 record) and the
    numpy fp32 recurrence (every fp32 REC / REC_CORR record) against the fp64 C oracle."""
    c = BY_ID[cid]
    p, u, lam, ref, sc, base = _ref(cid)
    models = [("numpy", FC.np_fk(c, p, u, lam, base=base), RTOL[torch.float64])]
    if c.dtype == "f32":
        models.append((("c32", c.path), FC.c_oracle_f32(c, p, u, lam), RTOL[torch.float32]))
        if c.path != FC.DIRECT:
            models.append((("rec32", c.path), FC.rec_model_f32(c, p, u, lam), RTOL[torch.float32]))
    for name, got, rtol in models:
        for k, what in enumerate(("du", "lamJ", "dp")):
            assert_close(got[k], ref[k], sc[k], rtol * SOUND[name][k], f"{name} {what}")


# least err/bound over the group, as measured (asserted with a factor 2 of slack below), and the group's size
MUTATION_LEAST = {
    "no_wrap": (694, 484), "generic_small": (1.1e4, 184), "exact_knots": (1.4e4, 205), "no_base_second": (71, 584),
    "dw_slot": (1.0e3, 1130), "skip_q": (4.1e3, 114), "first_trip": (2.8e4, 12),
}


@pytest.mark.parametrize("which", list(FC.MUTATIONS))
def test_discrimination(which):
    """Every wrong restatement leaves the bound (err/bound > 1 on du, λᵀJ or dp) in every record of its group."""
    group = [c for c in FC.CASES if FC.MUTATIONS[which](c)]
    least, missed = np.inf, {}
    for c in group:
        p, u, lam, ref, sc, base = _ref(c.id)
        got = FC.np_fk(c, p, u, lam, which, base=base)
        r = max(_ratio(got[k], ref[k], sc[k], RTOL[TDT[c.dtype]]) for k in range(3))
        least = min(least, r)
        if not r > 1.0:
            missed[c.id] = r
    print(f"{which}: least err/bound {least:.3g} over {len(group)} records")
    assert len(group) == MUTATION_LEAST[which][1]
    assert not missed, f"{which}: not told from the oracle in {len(missed)} of {len(group)} records: {missed}"
    assert least >= MUTATION_LEAST[which][0] / 2
