"""kanode_edge_scores (kan_score.hip; handle.edge_scores, KDense.edge_scores, Chain.edge_scores) and kanode.prune on
the GPU: scores[i, o] = max_k |φ_{o,i}(x_k)| against kanode_edge_activations (bit for bit where that kernel serves
the layer, out_dims <= 64) and against the oracle's O.edge_act at test_edge_activations_golden_and_identity's bar
(RTOL of Σ|terms| + 1e-3 of its maximum: |max_k a - max_k b| <= max_k |a - b|, so the per-element bar carries to
the maximum with the largest per-sample scale)."""
import numpy as np
import pytest
import torch

import sparse_cases as S
from gpu_util import RTOL, assert_close, chain_scale, device, t
from oracle import oracle as O

import kanode
from kanode import _lib as L

pytestmark = pytest.mark.gpu

SHAPES = [(2, 10, 5), (10, 2, 5), (3, 70, 5), (70, 3, 4)]
KS = [1, 63, 65, 141, 1000]
_KW = {"tanh_fast": dict(normalizer="tanh"), "softsign": dict(normalizer="softsign"),
       "rbf": dict(normalizer="tanh", basis_func="rbf"), "rswaf": dict(normalizer="tanh", basis_func="rswaf")}
_SPEC = {"tanh_fast": ("tanh_fast", "rbf"), "softsign": ("softsign", "rbf"), "rbf": ("tanh_fast", "rbf"),
         "rswaf": ("tanh_fast", "rswaf")}


def _case(I, O_, G, K, seed):
    rng = np.random.default_rng(seed)
    p = rng.uniform(-0.5, 0.5, O_ * G * I + O_ * I)
    x = rng.uniform(-1.0, 2.5, (K, I))
    return p, x


def _check(I, O_, G, K, kind, dtype):
    norm, basis = _SPEC[kind]
    spec = O.LayerSpec(I, O_, G, norm, basis)
    lay = kanode.KDense(I, O_, G, **_KW[kind])
    p, x = _case(I, O_, G, K, 100 * I + O_ + K)
    if dtype == torch.float32:
        p, x = p.astype(np.float32).astype(np.float64), x.astype(np.float32).astype(np.float64)
    pt, xt = t(p, dtype), t(x, dtype)
    sc = lay.edge_scores(xt, pt)
    assert sc.shape == (I, O_) and sc.dtype == dtype
    if O_ <= 64:
        act = lay.edge_activations(xt, pt)
        assert torch.equal(sc, act.abs().amax(0)), (I, O_, G, K, kind, dtype)
    ref = np.abs(O.edge_act(spec, p, x))
    scale = np.abs(O.edge_act(spec, np.abs(p), x))
    scale = (scale + 1e-3 * np.max(scale)).max(axis=0)
    assert_close(sc, ref.max(axis=0), scale, RTOL[dtype], f"scores {(I, O_, G, K, kind, dtype)}")


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("kind", ["tanh_fast", "softsign"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_edge_scores_match_the_activations_and_the_oracle(shape, kind, dtype):
    for K in KS:
        _check(*shape, K, kind, dtype)


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("kind", ["rbf", "rswaf"])
def test_edge_scores_other_bases(kind, dtype):
    """rbf on a non-default grid length (the corrected recurrence) and rswaf (the direct formula), at one shape."""
    for K in (65, 141):
        _check(3, 7, 8 if kind == "rbf" else 5, K, kind, dtype)


def test_edge_scores_many_samples_and_a_wide_layer():
    """K = 100000 on [2 -> 10] (the samples split over blocks, partial maxima and the reduction pass) and
    [10 -> 512] at K = 141 (the surrogate's second layer, which kanode_edge_activations refuses)."""
    rng = np.random.default_rng(7)
    lay = kanode.KDense(2, 10, 5)
    p, x = _case(2, 10, 5, 100000, 7)
    sc = lay.edge_scores(t(x), t(p))
    assert torch.equal(sc, lay.edge_activations(t(x), t(p)).abs().amax(0))
    wide = kanode.KDense(10, 512, 5)
    pw = rng.uniform(-0.5, 0.5, wide.parameterlength())
    xw = rng.uniform(-1.0, 2.5, (141, 10))
    with pytest.raises(L.KanodeError, match="out_dims <= 64"):
        wide.edge_activations(t(xw), t(pw))
    spec = O.LayerSpec(10, 512, 5, "tanh_fast")
    scale = np.abs(O.edge_act(spec, np.abs(pw), xw))
    scale = (scale + 1e-3 * np.max(scale)).max(axis=0)
    assert_close(wide.edge_scores(t(xw), t(pw)), np.abs(O.edge_act(spec, pw, xw)).max(axis=0), scale,
                 RTOL[torch.float64], "wide scores")


@pytest.mark.parametrize("shape", [(2, 10, 5), (3, 70, 5)], ids=["k_kernel", "o_kernel"])
@pytest.mark.parametrize("K", [141, 1000])
def test_a_nan_sample_marks_exactly_its_inputs_edges(shape, K):
    I, O_, G = shape
    lay = kanode.KDense(I, O_, G)
    p, x = _case(I, O_, G, K, 3)
    x[K // 2, 1] = np.nan
    sc = lay.edge_scores(t(x), t(p))
    nan = torch.isnan(sc)
    assert nan[1].all() and not nan[0].any() and not nan[2:].any()
    x[K // 2, 1] = 0.0
    clean = lay.edge_scores(t(x), t(p))
    assert torch.equal(clean[0], sc[0]) and not torch.isnan(clean).any()


def test_k_0_is_rejected():
    lay = kanode.KDense(2, 10, 5)
    p, _ = _case(2, 10, 5, 1, 1)
    with pytest.raises(L.KanodeError, match="K <= 0"):
        lay.edge_scores(torch.empty((0, 2), dtype=torch.float64, device=device()), t(p))


def test_chain_edge_scores_propagate_the_input():
    """Chain.edge_scores scores layer l on the output of layer l - 1 (Activation_getter.jl:39): equal to
    KDense.edge_scores on the layer forward's output, and within the bar of the oracle's propagated activations."""
    p, x = S.make(S.DEEP_DIMS, S.DEEP_DROPPED, seed=21)
    chain = kanode.Chain(*[kanode.KDense(i, o, 5) for i, o in zip(S.DEEP_DIMS[:-1], S.DEEP_DIMS[1:])])
    got = chain.edge_scores(t(x), t(p))
    acts = S.oracle_activations(S.DEEP_DIMS, p, x)
    h, off = t(x), 0
    for l, lay in enumerate(chain.layers):
        pl = t(p[off:off + lay.parameterlength()])
        assert torch.equal(got[l], lay.edge_scores(h, pl))
        ref = np.abs(acts[l]).max(axis=0)
        assert_close(got[l], ref, ref + 1e-3 * ref.max() + 1e-9, 1e-10, f"chain scores {l}")
        h, _ = lay(h, pl, None)
        off += lay.parameterlength()


def test_prune_end_to_end():
    """kanode.prune on test_sparse_cpu.py's construction: the oracle's kept set; ChainRHS of the pruned chain
    within 1e-13 of scale of the full chain with the dropped nodes zeroed; and the pruned [2, 7, 2] network trains
    through step() on the one-workgroup kernels with sparse_reg on the native step."""
    p, x = S.make(S.LV_DIMS, S.LV_DROPPED, seed=21)
    want, _ = S.driver_keep_rule(S.oracle_activations(S.LV_DIMS, p, x), S.THETA)
    chain = kanode.Chain(kanode.KDense(2, 10, 5), kanode.KDense(10, 2, 5))
    pruned, pp, kept = kanode.prune(chain, p, x, S.THETA, dtype=torch.float64, device=device())
    assert [k.tolist() for k in kept] == want and len(kept[0]) == 7
    assert [l.out_dims for l in pruned.layers] == [7, 2] and pp.shape == (pruned.parameterlength(),)
    rhs = kanode.ChainRHS(pruned, dtype=torch.float64, device=device())
    full = kanode.ChainRHS(chain, dtype=torch.float64, device=device())
    p_zero = S.touch_nodes(S.LV_DIMS, p, S.LV_DROPPED, 0.0)
    got = rhs.hd.rhs(t(pp), t(x))
    ref = full.hd.rhs(t(p_zero), t(x))
    assert_close(got, ref.cpu().numpy(), chain_scale(S.specs_for(S.LV_DIMS), p_zero, x), 1e-13, "pruned rhs")
    ts = [0.1 * i for i in range(35)]
    X = np.random.default_rng(2).uniform(0.5, 2.0, (35, 1, 2))
    tr = kanode.Trainer(rhs, t(np.array([[1.0, 1.0]])), (0.0, 3.5), ts, t(X), t(pp / 10), eta=1e-3, sparse_reg=5e-4)
    assert tr._native_run_path() is None            # (the device loop is the [2, 10, 2] kernel's alone)
    loss = tr.step()
    assert rhs.hd.get_option("last_adjoint") == L.ADJ_CHAIN_WG
    assert np.isfinite(loss) and torch.isfinite(tr.p).all()
