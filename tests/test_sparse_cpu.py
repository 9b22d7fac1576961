"""The host half of kanode.prune (kanode/sparse.py), without a GPU: the keep rule against the driver's loop restated
over the oracle's per-edge activations (LV_driver_KANODE.jl:76-84), and the parameter slicing against the full
chain with the dropped nodes' parameters set to zero."""
import numpy as np
import pytest

import sparse_cases as S
from gpu_util import chain_scale
from oracle import oracle as O

import kanode


def _kept_sets(dims, dropped):
    return [[j for j in range(dims[l + 1]) if j not in dropped[l]] for l in range(len(dropped))]


@pytest.mark.parametrize("dims,dropped", [(S.LV_DIMS, S.LV_DROPPED), (S.DEEP_DIMS, S.DEEP_DROPPED)])
def test_keep_rule_matches_the_driver(dims, dropped):
    """LV [2, 10, 2], G = 5, K = 141, θ = 1e-2: three hidden nodes at 1e-4 of the others' magnitudes.  No oracle
    node score lies in [θ/2, 2θ] (a condition on the inputs: the comparison cannot hinge on rounding), and
    prune_nodes on max_k |O.edge_act| keeps exactly the unscaled nodes, as the driver's loop does."""
    p, x = S.make(dims, dropped, seed=21)
    assert x.shape[0] == 141
    acts = S.oracle_activations(dims, p, x)
    want, node_scores = S.driver_keep_rule(acts, S.THETA)
    for sc in node_scores:
        print(np.sort(sc))
        assert not np.any((sc >= S.THETA / 2) & (sc <= 2 * S.THETA))
    scores = [np.abs(a).max(axis=0) for a in acts]            # (I, O): Chain.edge_scores' layout
    kept = kanode.prune_nodes(scores, S.THETA)
    assert [k.tolist() for k in kept] == want == _kept_sets(dims, dropped)
    if dims == S.LV_DIMS:
        assert len(kept[0]) == 7


@pytest.mark.parametrize("dims,dropped", [(S.LV_DIMS, S.LV_DROPPED), (S.DEEP_DIMS, S.DEEP_DROPPED)])
def test_parameter_slicing(dims, dropped):
    """The oracle chain at (pruned dims, p_pruned) against the full chain with the dropped nodes' parameters zeroed:
    within 1e-13 of Σ|terms| (gpu_util's scale)."""
    p, x = S.make(dims, dropped, seed=22)
    chain = kanode.Chain(*[kanode.KDense(i, o, 5) for i, o in zip(dims[:-1], dims[1:])])
    kept = _kept_sets(dims, dropped)
    pruned, pp = kanode.prune_params(chain, p, kept)
    pdims = [dims[0]] + [len(k) for k in kept] + [dims[-1]]
    assert [pruned[0].in_dims] + [l.out_dims for l in pruned.layers] == pdims
    assert pruned[0].normalizer == "tanh_fast" and pruned[0].denominator == chain[0].denominator
    assert isinstance(pp, np.ndarray) and pp.dtype == p.dtype and pp.shape == (pruned.parameterlength(),)
    if dims == S.LV_DIMS:
        assert pdims == [2, 7, 2]
    got = O.chain_fwd(S.specs_for(pdims), pp, x)
    p_zero = S.touch_nodes(dims, p, dropped, 0.0)
    ref = O.chain_fwd(S.specs_for(dims), p_zero, x)
    err = np.abs(got - ref)
    bound = 1e-13 * chain_scale(S.specs_for(dims), p_zero, x)
    print(dims, "max err", err.max(), "min bound", bound.min())
    assert np.all(err <= bound)
    # every kept parameter is the trained one, in place: spot-check the two layouts directly
    G = 5
    full, cut = S.layer_views(dims, p), S.layer_views(pdims, pp)
    assert np.array_equal(cut[0][0], full[0][0][kept[0], :]) and np.array_equal(cut[0][1], full[0][1][kept[0], :])
    cols = np.concatenate([np.arange(G) + G * j for j in kept[0]])
    rows1 = kept[1] if len(kept) > 1 else list(range(dims[2]))
    assert np.array_equal(cut[1][0], full[1][0][np.ix_(rows1, cols)])
    assert np.array_equal(cut[1][1], full[1][1][np.ix_(rows1, kept[0])])


def test_prune_params_keeps_a_tensor_a_tensor():
    import torch
    p, _ = S.make(S.LV_DIMS, S.LV_DROPPED, seed=23)
    chain = kanode.Chain(kanode.KDense(2, 10, 5), kanode.KDense(10, 2, 5))
    kept = _kept_sets(S.LV_DIMS, S.LV_DROPPED)
    _, pn = kanode.prune_params(chain, p, kept)
    _, pt = kanode.prune_params(chain, torch.as_tensor(p, dtype=torch.float32), kept)
    assert isinstance(pt, torch.Tensor) and pt.dtype == torch.float32
    assert np.array_equal(pt.numpy(), pn.astype(np.float32))


def test_bindings_declare_the_new_entry_points():
    """The header, the ctypes table and the Julia shim (textually: Julia is not run here) carry the penalty setter,
    the scores entry and prune; train_tsit5! takes the l1 keyword and restores the handle's penalty."""
    import os
    import re
    from conftest import ROOT
    from kanode import _lib as L
    hdr = open(os.path.join(ROOT, "include", "kanode.h")).read()
    jl = open(os.path.join(ROOT, "julia", "KANODEHip.jl")).read()
    names = {n for n, _, _ in L.SIGNATURES}
    for sym in ("kanode_set_l1_penalty", "kanode_get_l1_penalty", "kanode_edge_scores"):
        assert re.search(r"\b" + sym + r"\s*\(", hdr) and sym in names and ":" + sym in jl, sym
    for pat in (r"^set_l1_penalty!\(h::Handle, λ::Real\)", r"^function edge_scores\(l::KANChainHip,",
                r"^function prune_nodes\(", r"^function prune\(l::KANChainHip,"):
        assert re.search(pat, jl, re.M), pat
    body = re.search(r"^function train_tsit5!\(.*?^end\b", jl, re.S | re.M).group(0)
    assert "l1::Real = 0.0" in body and body.index("set_l1_penalty!(h, l1)") < body.index(":kanode_train_tsit5")
    assert "finally" in body and "set_l1_penalty!(h, old)" in body
    lib = kanode.lib()
    assert lib.kanode_set_l1_penalty(None, 1.0) == L.ERR_INVALID_ARG and lib.kanode_get_l1_penalty(None) == 0.0
    assert lib.kanode_edge_scores(None, 0, None, None, None, 1, None) == L.ERR_INVALID_ARG


def test_errors():
    """ValueError when every node of a layer falls, and on a score that is not finite."""
    p, x = S.make(S.LV_DIMS, S.LV_DROPPED, seed=21)
    scores = [np.abs(a).max(axis=0) for a in S.oracle_activations(S.LV_DIMS, p, x)]
    with pytest.raises(ValueError, match="every node"):
        kanode.prune_nodes(scores, 1e3)
    bad = [s.copy() for s in scores]
    bad[1][3, 0] = np.nan
    with pytest.raises(ValueError, match="not finite"):
        kanode.prune_nodes(bad, S.THETA)
    bad[1][3, 0] = np.inf
    with pytest.raises(ValueError, match="not finite"):
        kanode.prune_nodes(bad, S.THETA)
    with pytest.raises(ValueError, match="at least 2 layers"):
        kanode.prune_nodes(scores[:1], S.THETA)
    chain = kanode.Chain(kanode.KDense(2, 10, 5), kanode.KDense(10, 2, 5))
    with pytest.raises(ValueError, match="lose every node"):
        kanode.prune_params(chain, p, [[]])
    with pytest.raises(ValueError, match="ascending"):
        kanode.prune_params(chain, p, [[3, 3]])
    with pytest.raises(ValueError, match="ascending"):
        kanode.prune_params(chain, p, [[0, 10]])
