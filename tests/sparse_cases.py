"""The networks the pruning tests share (test_sparse_cpu.py, test_gpu_prune.py): a chain whose hidden nodes are
either negligible (every parameter that touches the node scaled by 1e-4) or plainly alive (magnitudes in
[0.3, 0.6], random signs), the driver's keep rule restated in numpy over the oracle's per-edge activations
(LV_driver_KANODE.jl:76-84), and the full chain with the dropped nodes' parameters set to zero."""
import numpy as np

from oracle import oracle as O

THETA = 1e-2


def specs_for(dims, G=5, normalizer="tanh_fast"):
    return [O.LayerSpec(i, o, G, normalizer) for i, o in zip(dims[:-1], dims[1:])]


def layer_views(dims, p, G=5):
    """[(C [O, G·I], W [O, I])] as writable views into the flat ComponentArray vector p."""
    out, off = [], 0
    for I, O_ in zip(dims[:-1], dims[1:]):
        nC, nW = O_ * G * I, O_ * I
        C = p[off:off + nC].reshape(G * I, O_).T
        W = p[off + nC:off + nC + nW].reshape(I, O_).T
        out.append((C, W))
        off += nC + nW
    assert off == p.size
    return out


def touch_nodes(dims, p, dropped, factor, G=5):
    """Multiply by `factor` every parameter of the hidden nodes dropped[l] (layer l's rows, layer l + 1's column
    blocks g + G·j and W columns); returns a new vector."""
    q = p.copy()
    lv = layer_views(dims, q, G)
    for l, nodes in enumerate(dropped):
        for j in nodes:
            lv[l][0][j, :] *= factor
            lv[l][1][j, :] *= factor
            lv[l + 1][0][:, G * j:G * j + G] *= factor
            lv[l + 1][1][:, j] *= factor
    return q


def make(dims, dropped, seed, K=141, G=5):
    """(p, x): magnitudes in [0.3, 0.6] with random signs, the nodes dropped[l] of hidden layer l scaled by 1e-4;
    x (K, dims[0]) uniform in [0.5, 2) (the Lotka-Volterra state range)."""
    rng = np.random.default_rng(seed)
    P = sum(s.param_length() for s in specs_for(dims, G))
    p = rng.uniform(0.3, 0.6, P) * rng.choice([-1.0, 1.0], P)
    x = rng.uniform(0.5, 2.0, (K, dims[0]))
    return touch_nodes(dims, p, dropped, 1e-4, G), x


def oracle_activations(dims, p, x, G=5):
    """[act_l (K, I_l, O_l)]: O.edge_act of every layer, the input propagated with O.layer_fwd."""
    specs = specs_for(dims, G)
    acts, off, h = [], 0, x
    for s in specs:
        pl = p[off:off + s.param_length()]
        acts.append(O.edge_act(s, pl, h))
        h = O.layer_fwd(s, pl, h)
        off += s.param_length()
    return acts


def driver_keep_rule(acts, theta=THETA):
    """The loop of LV_driver_KANODE.jl:76-84 for every hidden layer: (kept, node scores), node score =
    min(input_score, output_score)."""
    kept, scores = [], []
    for l in range(len(acts) - 1):
        keep, sc = [], []
        for j in range(acts[l].shape[2]):
            input_score = max(np.max(np.abs(acts[l][:, i, j])) for i in range(acts[l].shape[1]))
            output_score = np.max(np.abs(acts[l + 1][:, j, :]))
            sc.append(min(input_score, output_score))
            if min(input_score, output_score) > theta:
                keep.append(j)
        kept.append(keep)
        scores.append(np.array(sc))
    return kept, scores


# the Lotka-Volterra network of the driver, three negligible hidden nodes
LV_DIMS, LV_DROPPED = [2, 10, 2], [[1, 4, 8]]
# three layers, nodes dropped in both hidden layers
DEEP_DIMS, DEEP_DROPPED = [3, 6, 5, 2], [[0, 3], [2]]
