"""Pruning of a sparsified KAN (the step after training with sparse_on = 1; LV_driver_KANODE.jl:52-108).

    prune_nodes(scores, theta)      — the keep rule on per-edge scores (host, no GPU)
    prune_params(chain, p, kept)    — the narrower Chain and its parameters (host, no GPU)
    prune(chain, p, x, theta)       — Chain.edge_scores on the device (kanode_edge_scores), then the two above

A hidden node j of layer l is kept iff min(max_i scores_l[i, j], max_o scores_{l+1}[j, o]) > theta, with
scores_l[i, o] = max_k |φ_{o,i}(x_k)| on the unpruned network (:76-84: input_score / output_score from
activation_getter).  Unlike the reference's prune, which slices the freshly initialised global pM (:96-104) and fills
layer 2's W from its C (:104), the kept nodes keep their trained C and W.
"""
from __future__ import annotations

import numpy as np
import torch

from .layers import Chain, KDense


def _np(a) -> np.ndarray:
    return a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)


def prune_nodes(scores, theta: float = 1e-2) -> list:
    """kept[l] (ascending int64 indices) for every hidden layer l = 0 .. L-2 of a chain of L >= 2 layers, from
    scores[l] of shape (I_l, O_l) (Chain.edge_scores' list).  ValueError if any score is not finite (a diverged
    network must not be pruned) or a layer would lose every node."""
    sc = [_np(s).astype(np.float64) for s in scores]
    if len(sc) < 2:
        raise ValueError("prune needs a chain of at least 2 layers")
    for l, s in enumerate(sc):
        if s.ndim != 2 or (l > 0 and s.shape[0] != sc[l - 1].shape[1]):
            raise ValueError(f"scores[{l}] has shape {s.shape}: expected (in_dims, out_dims) of consecutive layers")
        if not np.all(np.isfinite(s)):
            raise ValueError(f"prune: layer {l} has a score that is not finite")
    kept = []
    for l in range(len(sc) - 1):
        in_score = sc[l].max(axis=0)          # over the inputs i of layer l
        out_score = sc[l + 1].max(axis=1)     # over the outputs o of layer l + 1
        k = np.nonzero(np.minimum(in_score, out_score) > theta)[0].astype(np.int64)
        if k.size == 0:
            raise ValueError(f"prune: every node of hidden layer {l} scores at most theta = {theta}")
        kept.append(k)
    return kept


def prune_params(chain: Chain, p, kept):
    """(chain_pruned, p_pruned): hidden layer l narrowed to the nodes kept[l].  In the ComponentArray layout
    (C [O, G·I] column-major, then W [O, I]) layer l keeps the rows kept[l] of C and W, layer l + 1 the column blocks
    g + G·j of C and the columns j of W for j in kept[l].  p_pruned has p's type (numpy dtype, or torch dtype and
    device)."""
    L = len(chain)
    if L < 2 or len(kept) != L - 1:
        raise ValueError("prune_params: kept needs one index list per hidden layer of a chain of >= 2 layers")
    kept = [np.asarray(k, dtype=np.int64).reshape(-1) for k in kept]
    for l, k in enumerate(kept):
        if k.size == 0:
            raise ValueError(f"prune_params: hidden layer {l} would lose every node")
        if np.any(k < 0) or np.any(k >= chain[l].out_dims) or np.any(np.diff(k) <= 0):
            raise ValueError(f"prune_params: kept[{l}] must be ascending indices below {chain[l].out_dims}")
    pn = _np(p)
    if pn.shape != (chain.parameterlength(),):
        raise ValueError(f"p has shape {pn.shape}, expected ({chain.parameterlength()},)")
    layers, pm = [], []
    for l, (lay, q) in enumerate(zip(chain.layers, chain.unflatten(pn))):
        G = lay.grid_len
        C = np.asarray(q["C"])
        W = np.asarray(q["W"]) if lay.use_base_act else None
        I, O = lay.in_dims, lay.out_dims
        if l > 0:
            cols = (np.arange(G)[None, :] + G * kept[l - 1][:, None]).reshape(-1)
            C = C[:, cols]
            W = W[:, kept[l - 1]] if W is not None else None
            I = kept[l - 1].size
        if l < L - 1:
            C = C[kept[l], :]
            W = W[kept[l], :] if W is not None else None
            O = kept[l].size
        layers.append(KDense(I, O, G, normalizer=lay.normalizer, grid_lims=lay.grid_lims,
                             denominator=lay.denominator, basis_func=lay.basis_func, base_act=lay.base_act,
                             use_base_act=lay.use_base_act, init_C=lay.init_C, init_W=lay.init_W,
                             allow_fast_activation=False))
        pm.append({"C": C, "W": W} if W is not None else {"C": C})
    pruned = Chain(*layers)
    pp = pruned.flatten(pm).astype(pn.dtype, copy=False)
    if isinstance(p, torch.Tensor):
        return pruned, torch.as_tensor(pp, dtype=p.dtype, device=p.device)
    return pruned, pp


def prune(chain: Chain, p, x, theta: float = 1e-2, *, dtype=torch.float64, device=None):
    """(chain_pruned, p_pruned, kept) of a chain of >= 2 KDense layers at the samples x (K, I_0): the scores come
    from Chain.edge_scores on `device` (kanode_edge_scores, in `dtype`), all on the unpruned network."""
    dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    xt = torch.as_tensor(_np(x) if not isinstance(x, torch.Tensor) else x).to(device=dev, dtype=dtype)
    pt = torch.as_tensor(_np(p) if not isinstance(p, torch.Tensor) else p).to(device=dev, dtype=dtype)
    kept = prune_nodes(chain.edge_scores(xt.reshape(-1, chain[0].in_dims).contiguous(), pt.contiguous()), theta)
    pruned, pp = prune_params(chain, p, kept)
    return pruned, pp, kept
