"""One handle and one dense solution reused across calls whose storage needs go up, down and up again
(n_save 3 -> 40 -> 3 -> 64, tf 0.5 -> 3.5 -> 0.5 -> 3.5, so saveat staging, step records and dense-output slots
all regrow and are then used below their capacity): every result is bitwise what the same call gives on a
fresh handle and a fresh solution.  One case per driver of kanode_solve_tsit5 / kanode_adjoint_tsit5 that owns
storage, at the smallest shape that reaches it, plus kanode_forward_sensitivity_tsit5."""
import numpy as np
import pytest
import torch

from gpu_util import device, t

import kanode
from kanode import _lib as L

pytestmark = pytest.mark.gpu

CALLS = [(3, 0.5), (40, 3.5), (3, 0.5), (64, 3.5)]   # (n_save, tf)


def lv():
    return kanode.ChainRHS(kanode.Chain(kanode.KDense(2, 10, 5), kanode.KDense(10, 2, 5)), device=device())


def fk(nx):
    kan1 = kanode.Chain(kanode.KDense(1, 1, 10, normalizer="softsign"))
    return kanode.FisherKPPRHS(kan1, nx=nx, dx=1.0 / (nx - 1), D=0.01, device=device())


def fk_u0(nx, B):
    rng = np.random.default_rng(2)
    x = np.arange(nx) / (nx - 1)
    c, d, a = rng.uniform(0.3, 0.7, (B, 1)), rng.uniform(0.1, 0.3, (B, 1)), rng.uniform(0.5, 1, (B, 1))
    return a * (np.tanh((x - (c - d / 2)) / (d / 10)) - np.tanh((x - (c + d / 2)) / (d / 10))) / 2


LV_U0 = np.array([[1.0, 1.0], [0.7, 1.3], [1.5, 0.6]])
LV_OPT = dict(abstol=1e-7, reltol=1e-6)
# name: (make rhs, u0, P, scale of p, solver options, expected adjoint path or None)
CASES = {
    "lv_b1_onewg": (lv, LV_U0[:1], 240, 0.3, dict(LV_OPT), L.ADJ_CHAIN_WG),
    "lv_b3_onewg": (lv, LV_U0, 240, 0.3, dict(LV_OPT), L.ADJ_CHAIN_WG),
    "lv_host": (lv, LV_U0, 240, 0.3, dict(LV_OPT, control="host"), L.ADJ_HOST_LOOP),
    "lv_graph": (lv, LV_U0, 240, 0.3, dict(LV_OPT, control="device", graph_steps=4), L.ADJ_HOST_LOOP),
    "fk26_onewg": (lambda: fk(26), fk_u0(26, 1), 11, 1.0, dict(abstol=1e-8, reltol=1e-7), None),
    "fk128_loop": (lambda: fk(128), fk_u0(128, 6), 11, 1.0, dict(abstol=1e-6, reltol=1e-4), L.ADJ_HOST_LOOP),
}


def _saveat(n_save, tf):
    return [float(x) for x in np.linspace(0.0, tf, n_save)]


def _solve_and_adjoint(rhs, dense, u0, p, n_save, tf, opt):
    """One forward solve into `dense` (None: a fresh solution) and its adjoint; every output and count."""
    hd = rhs.hd
    if dense is not None:
        hd.release_dense(dense)   # the next solve takes it from the pool
    o = opt.to_c()
    u_save, st, dense = hd.solve_tsit5(p, u0, 0.0, tf, _saveat(n_save, tf), o, keep_dense=True)
    ts, dts = dense.step_sizes()
    dl = t(np.random.default_rng(n_save).normal(size=tuple(u_save.shape)))
    du0, dp, ast = hd.adjoint_tsit5(p, dense, dl, o, tuple(u0.shape))
    torch.cuda.synchronize()
    return dense, dict(u_save=u_save, du0=du0, dp=dp, ts=ts, dts=dts, stats=st, adjoint_stats=ast,
                       path=hd.get_option("last_adjoint"))


def _assert_same(got, ref, what):
    for k, r in ref.items():
        g = got[k]
        if isinstance(r, torch.Tensor):
            assert torch.equal(g, r), f"{what}: {k} differs (max {(g - r).abs().max().item():.3g})"
        elif isinstance(r, np.ndarray):
            assert g.shape == r.shape and np.array_equal(g, r), f"{what}: {k} differs"
        else:
            assert g == r, f"{what}: {k}: {g} != {r}"


@pytest.mark.parametrize("name", list(CASES))
def test_reused_solution_matches_fresh(name):
    make, u0, P, scale, okw, path = CASES[name]
    opt = kanode.Tsit5Options(**okw)
    u0 = t(u0)
    p = t(np.random.default_rng(7).uniform(-scale, scale, P))
    rhs, dense = make(), None
    steps = []
    for n_save, tf in CALLS:
        dense_before = dense
        dense, got = _solve_and_adjoint(rhs, dense, u0, p, n_save, tf, opt)
        assert dense_before is None or dense is dense_before      # the same solution object, reused
        _, ref = _solve_and_adjoint(make(), None, u0, p, n_save, tf, opt)
        _assert_same(got, ref, f"{name} n_save={n_save} tf={tf}")
        assert len(got["ts"]) == got["stats"]["naccept"] > 0
        if path is not None:
            assert got["path"] == path
        steps.append(got["stats"]["naccept"])
    assert steps[1] > steps[0] and steps[2] == steps[0] and steps[3] == steps[1]   # the storage need went up and down


def test_reused_forward_sensitivity_matches_fresh():
    opt = kanode.Tsit5Options(abstol=1e-8, reltol=1e-7)
    u0 = t(fk_u0(26, 1))
    p = t(np.random.default_rng(7).uniform(-1.0, 1.0, 11))

    def run(rhs, n_save, tf):
        u_save, s_save, st = rhs.hd.forward_sensitivity_tsit5(p, u0, 0.0, tf, _saveat(n_save, tf), opt.to_c())
        ts, dts = rhs.hd.forward_sensitivity_step_sizes()
        torch.cuda.synchronize()
        return dict(u_save=u_save, s_save=s_save, ts=ts, dts=dts, stats=st)

    rhs = fk(26)
    assert rhs.hd.forward_sensitivity_supported(1)
    for n_save, tf in CALLS[:3]:
        got = run(rhs, n_save, tf)
        _assert_same(got, run(fk(26), n_save, tf), f"fsens n_save={n_save} tf={tf}")
        assert len(got["ts"]) == got["stats"]["naccept"] > 0
