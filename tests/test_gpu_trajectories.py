"""The trajectory ensemble: R initial conditions of one problem at one p in one launch, a 16-lane row per trajectory
and every trajectory an ODE of its own (kanode_solve_trajectories_tsit5; KanodeHandle.solve_trajectories_tsit5,
kanode.solve_trajectories).  Trajectory r runs the batch-1 solve's device code (onewg_tsit5's ROW mode, the error
norm summed in the batch-1 kernel's order), so "equal" here is torch.equal on u[:, r:r+1, :] and == on the three
counts, against hd.solve_tsit5(p, u0[r:r+1]) on the same handle.

The chain shapes, their data and solver settings are tests/test_gpu_train_wg.py's, the Lotka-Volterra handle and P0
tests/test_gpu_train_loop.py's.  p = 3·data(sid)[0] and u0 = default_rng(21).uniform(0.5, 2.0, (9, N)): nine
trajectories are two full waves and one wave with a single live row."""
import ctypes as C

import numpy as np
import pytest
import torch

import test_gpu_train_wg as WG
from gpu_util import device, t
from test_gpu_train_loop import P0, lv

import kanode
from kanode import _lib as L
from kanode.handle import _ptr, _stream

pytestmark = pytest.mark.gpu

TS, OPTS = WG.TS, WG.OPTS
SPAN = (0.0, 3.5)
_RHS = {}


def opts(name, **kw):
    return kanode.Tsit5Options(**dict(OPTS[name], **kw))


def chain_rhs(sid, dtype=torch.float64):
    if (sid, dtype) not in _RHS:
        _RHS[(sid, dtype)] = lv(dtype) if sid == "LV" else WG.make_rhs(sid, dtype)
    return _RHS[(sid, dtype)]


def problem(sid, dtype=torch.float64, R=9):
    """(rhs, p, u0 [R, N])"""
    rhs = chain_rhs(sid, dtype)
    p = P0 if sid == "LV" else 3.0 * WG.data(sid)[0]
    u0 = np.random.default_rng(21).uniform(0.5, 2.0, (R, rhs.hd.N))
    return rhs, t(p, dtype), t(u0, dtype)


def single(hd, p, u0, r, tspan, saveat, o):
    return hd.solve_tsit5(p, u0[r:r + 1].contiguous(), tspan[0], tspan[1], saveat, o.to_c())[:2]


def same_as_single(hd, p, u0, tspan, saveat, o, what="", which=None):
    """One call; every trajectory (or those of `which`) equal to its own batch-1 solve_tsit5 on the same handle."""
    u, stats, stop = hd.solve_trajectories_tsit5(p, u0, tspan[0], tspan[1], saveat, o.to_c())
    R = u0.shape[0]
    assert u.shape == (len(saveat), R, u0.shape[1]) and stop == ["ok"] * R
    assert torch.isfinite(u).all()
    for r in (range(R) if which is None else which):
        one, st = single(hd, p, u0, r, tspan, saveat, o)
        ur = u[:, r:r + 1, :]
        print(what, r, stats[r], st, "bitwise" if torch.equal(ur, one) else (ur - one).abs().max().item())
        assert stats[r] == st
        assert torch.equal(ur, one)
    return u, stats


CASES = ([(s, o, torch.float64) for s in ("S1", "S4", "S5", "S6") for o in ("fixed", "default")] +
         [("S1", "tight", torch.float64), ("S4", "tight", torch.float64)] +
         [("S6", o, torch.float32) for o in ("fixed", "default")] + [("LV", "default", torch.float64)])


@pytest.mark.parametrize("sid,opt,dtype", CASES, ids=[f"{s}-{o}-{str(d)[-2:]}" for s, o, d in CASES])
def test_every_trajectory_equals_its_own_solve(sid, opt, dtype):
    rhs, p, u0 = problem(sid, dtype)
    assert rhs.hd.solve_trajectories_supported()
    u, _ = same_as_single(rhs.hd, p, u0, SPAN, TS, opts(opt), f"{sid} {opt}")
    assert not torch.equal(u[:, 0], u[:, 1])


def test_not_the_batched_solve():
    """S1 at the default tolerances: the batched solve() of the nine rows is ONE ODE with one step size (24 steps on
    the CPU oracle); on their own the nine take 19 to 22 accepted steps there, six with a rejected step and three
    without (tests/test_trajectories_cpu.py).  The device's last-bit differences can move a count by one, not all
    nine onto one value."""
    rhs, p, u0 = problem("S1")
    o = opts("default")
    u, stats, stop = rhs.hd.solve_trajectories_tsit5(p, u0, 0.0, 3.5, TS, o.to_c())
    batched, bst, _ = rhs.hd.solve_tsit5(p, u0, 0.0, 3.5, TS, o.to_c())
    nacc = [s["naccept"] for s in stats]
    nrej = [s["nreject"] for s in stats]
    print("naccept", nacc, "nreject", nrej, "batched", bst)
    assert stop == ["ok"] * 9
    assert len(set(nacc)) >= 2
    assert any(x == 0 for x in nrej) and any(x > 0 for x in nrej)
    assert u.shape == batched.shape and not torch.equal(u, batched)


def test_anchor_against_the_python_statement_on_the_cpu():
    """S1, fixed step, trajectory 4 against kanode.solve on the CPU oracle's RHS: the same 350 steps, values within
    1e-11 (the project's native-against-Python-statement bar)."""
    from oracle.oracle_rhs import OracleChainRHS
    rhs, p, u0 = problem("S1")
    o = opts("fixed")
    u, stats, stop = rhs.hd.solve_trajectories_tsit5(p, u0, 0.0, 3.5, TS, o.to_c())
    ref = kanode.solve(OracleChainRHS(WG.specs_of("S1")), u0[4:5].cpu(), SPAN, p.cpu(), TS, o)
    err = (u[:, 4:5, :].cpu() - ref.u).abs().max().item()
    print("anchor", stats[4], ref.stats, err)
    assert stats[4] == ref.stats and stats[4]["naccept"] == 350
    assert err <= 1e-11


def raw(hd, p, u0, tspan, saveat, n_save=None, R=None, u_save=None, p_null=False, o=None):
    """The C entry itself: (status, u_save, stats, stop)."""
    n = u0.shape[0]
    R = n if R is None else R
    n_save = len(saveat) if n_save is None else n_save
    if u_save is None:
        u_save = torch.full((max(len(saveat), 1), n, u0.shape[1]), -7.0, dtype=u0.dtype, device=u0.device)
    sv = (C.c_double * max(1, len(saveat)))(*saveat)
    st = (L.SolveStatsC * n)()
    stop = (C.c_int32 * n)()
    oc = (o or kanode.Tsit5Options()).to_c()
    rc = L.lib().kanode_solve_trajectories_tsit5(hd._h, None if p_null else _ptr(p), _ptr(u0), R, tspan[0], tspan[1],
                                                 sv, n_save, _ptr(u_save), C.byref(oc), st, stop, _stream(hd.device))
    torch.cuda.synchronize()
    return rc, u_save, st, stop


def test_one_row_stops_and_its_wave_mates_finish():
    """tests/test_trajectories_cpu.py's case (rows 1 and 6 scaled by 8, maxiters = 12: 3 against at least 19
    iterations): the stopped rows share their waves with rows that finish."""
    rhs, p, u0 = problem("S1")
    u0 = u0.clone()
    u0[[1, 6]] *= 8.0
    o = opts("default", maxiters=12)
    done = (1, 6)
    rc, u, st, stop = raw(rhs.hd, p, u0, SPAN, TS, o=o)
    assert rc == L.OK
    assert "trajectory 0:" in L.lib().kanode_last_error(rhs.hd._h).decode()
    print([(s.naccept, s.nreject) for s in st], list(stop))
    assert [int(x) for x in stop] == [0 if r in done else 1 for r in range(9)]
    for r in range(9):
        col = u[:, r, :]
        if r in done:
            one, s1 = single(rhs.hd, p, u0, r, SPAN, TS, o)
            assert torch.equal(u[:, r:r + 1, :], one)
            assert dict(naccept=st[r].naccept, nreject=st[r].nreject, nf=st[r].nf) == s1
            continue
        assert st[r].naccept + st[r].nreject == 12
        # the -7 fill: written up to the last stop the trajectory reached, untouched past it
        filled = (col == -7.0).all(dim=1).cpu()
        first = int(filled.nonzero()[0]) if filled.any() else len(TS)
        assert 1 <= first < len(TS) and filled[first:].all() and not (col[:first] == -7.0).any()
        assert torch.isfinite(col[:first]).all()
    with pytest.raises(L.KanodeError, match="maxiters"):
        kanode.solve(rhs, u0[0:1], SPAN, p, TS, o)
    sol = kanode.solve_trajectories(rhs, u0, SPAN, p, TS, o)
    assert sol.path == "device" and sol.stop == ["ok" if r in done else "maxiters" for r in range(9)]
    for r in range(9):
        if r in done:
            assert torch.equal(sol.u[:, r], u[:, r])
        else:
            assert torch.isnan(sol.u[:, r]).all()


@pytest.mark.parametrize("R", [1, 3, 4, 5, 9])
def test_partly_filled_waves(R):
    rhs, p, u0 = problem("S1", R=R)
    sv = [0.0, 0.02, 0.04]
    _, stats = same_as_single(rhs.hd, p, u0, (0.0, 0.04), sv, opts("fixed"), f"R={R}")
    assert all(s["naccept"] == 4 for s in stats)


def test_more_workgroups_than_compute_units():
    """R = 1030: 258 one-wave workgroups on 256 compute units, the last wave with two live rows.  A short span: the
    check is the indexing."""
    rhs, p, u0 = problem("LV", R=1030)
    sv = [0.0, 0.02, 0.04]
    u, stats = same_as_single(rhs.hd, p, u0, (0.0, 0.04), sv, opts("fixed"), "R=1030", which=(0, 1, 1027, 1029))
    assert torch.equal(u[0], u0) and all(s == stats[0] for s in stats)


def test_saveat_at_the_ends_only():
    rhs, p, u0 = problem("S1")
    u, _ = same_as_single(rhs.hd, p, u0, SPAN, [0.0, 3.5], opts("default"), "ends")
    assert torch.equal(u[0], u0)


_NOT_COVERED = []


def not_covered():
    """(name, rhs, p, u0 [3, N]) of handles the trajectory solve does not take (made once)."""
    if not _NOT_COVERED:
        rng = np.random.default_rng(5)
        wide = kanode.ChainRHS(kanode.Chain(kanode.KDense(2, 20, 5), kanode.KDense(20, 2, 5)), dtype=torch.float64,
                               device=device())
        _NOT_COVERED.append(("[2,20,2]", wide, t(rng.uniform(-0.1, 0.1, wide.hd.P)), t(rng.uniform(0.5, 2.0, (3, 2)))))
        nx = 26
        kan1 = kanode.Chain(kanode.KDense(1, 1, 10, normalizer="softsign", basis_func="rbf"))
        fk = kanode.FisherKPPRHS(kan1, nx=nx, dx=1.0 / nx, D=0.01, dtype=torch.float64, device=device())
        x = np.arange(nx) / nx
        c = np.array([[0.4], [0.5], [0.6]])
        d = np.abs(x[None, :] - c)
        fu0 = np.exp(-(np.minimum(d, 1.0 - d) / 0.15) ** 2)
        _NOT_COVERED.append(("fisher-kpp", fk, t(rng.normal(0.0, 0.3, 11)), t(fu0)))
    return _NOT_COVERED


def refused_and_host(name, rhs, p, u0):
    sv = [0.0, 0.25, 0.5]
    assert not rhs.hd.solve_trajectories_supported()
    rc, u_save, _, _ = raw(rhs.hd, p, u0, (0.0, 0.5), sv)
    assert rc == L.ERR_UNSUPPORTED and "not supported" in L.lib().kanode_last_error(rhs.hd._h).decode(), name
    assert (u_save == -7.0).all()
    with pytest.raises(L.KanodeError, match="not supported"):
        rhs.hd.solve_trajectories_tsit5(p, u0, 0.0, 0.5, sv, kanode.Tsit5Options().to_c())
    sol = kanode.solve_trajectories(rhs, u0, (0.0, 0.5), p, sv)
    R = u0.shape[0]
    assert sol.path == "host" and sol.stop == ["ok"] * R and sol.u.shape == (3, R, u0.shape[1])
    for r in range(R):
        one = kanode.solve(rhs, u0[r:r + 1], (0.0, 0.5), p, sv)
        assert torch.equal(sol.u[:, r:r + 1, :], one.u) and sol.stats[r] == one.stats


@pytest.mark.parametrize("which", range(2))
def test_not_covered_is_refused_and_takes_the_host_path(which):
    refused_and_host(*not_covered()[which])


def test_fused_solve_off_is_not_covered():
    rhs, p, u0 = problem("LV", R=3)
    with rhs.hd.options(fused_solve=0):
        refused_and_host("fused_solve=0", rhs, p, u0)
    assert rhs.hd.solve_trajectories_supported()


def test_bad_arguments():
    rhs, p, u0 = problem("LV", R=3)
    sv = [0.0, 0.25, 0.5]
    for kw in (dict(R=0), dict(R=65537), dict(p_null=True), dict(n_save=0)):
        rc, u_save, _, _ = raw(rhs.hd, p, u0, (0.0, 0.5), sv, **kw)
        assert rc == L.ERR_INVALID_ARG and (u_save == -7.0).all(), kw
    rc, u_save, _, _ = raw(rhs.hd, p, u0, (0.0, 0.5), [0.5, 0.25, 0.0])
    assert rc == L.ERR_INVALID_ARG and (u_save == -7.0).all()
    rc, u_save, _, _ = raw(rhs.hd, p, u0, (0.0, 0.5), sv)
    assert rc == L.OK and torch.isfinite(u_save).all() and not (u_save == -7.0).any()


def test_the_handle_is_left_as_it_was():
    rhs, p, u0 = problem("LV")
    o = opts("default")
    a = kanode.solve(rhs, u0, SPAN, p, TS, o)
    one = kanode.solve(rhs, u0[2:3], SPAN, p, TS, o)
    sol = kanode.solve_trajectories(rhs, u0, SPAN, p, TS, o)
    assert sol.path == "device" and torch.equal(sol.u[:, 2:3, :], one.u)
    b = kanode.solve(rhs, u0, SPAN, p, TS, o)
    assert torch.equal(a.u, b.u) and a.stats == b.stats
    assert not torch.equal(sol.u, a.u)
