#!/usr/bin/env python
"""Replica-iterations per second of ensemble training (kanode.EnsembleTrainer: R replicas, one workgroup each, one
launch per chunk) against R Trainer.run calls one after another and against the C port, on two problems:
  lv   tools/bench_lv1_train.py's Lotka-Volterra trajectory (kanode_train_ensemble_tsit5), without the test solve
  fk   tools/bench_fk26_train.py's Fisher-KPP field (26, 1, G = 10) (kanode_train_forward_ensemble_tsit5)

For every R of --replicas the two legs run in turn, round after round (interleaved), each from fresh trainers
(replica r starts from p0 scaled by 1 + 1e-4·r), --iters iterations in one launch per call:
  ens   EnsembleTrainer.run(iters, chunk=iters)                    one launch of R workgroups
  seq   R times Trainer.run(iters, chunk=iters), one after another R launches of one workgroup
A leg's figure is the median over the rounds, and its spread (max - min)/median over those rounds is the margin
any comparison between legs is read against.  The C port (oracle: chain_epoch / fk_fsens_epoch) is timed on one core;
"16 cores" is that time for ceil(R / 16) rounds of replicas, computed, not run.

--legs seq --replicas 1 uses only API an older build has, so the same script times Trainer.run there
(--pkg DIR: the directory holding that build's `kanode` package, its libkanode.so inside).
Prints one JSON line; --out writes it to a file as well.

    python tools/bench_ensemble.py [--problems lv,fk] [--replicas 1,16,64,256,512] [--iters 16] [--rounds 7]
                                   [--legs ens,seq] [--no-cpu] [--pkg DIR] [--out FILE]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def lv_problem(kanode, dev):
    from scipy.integrate import solve_ivp
    ts = [0.1 * i for i in range(35)]
    f = lambda t, x: [1.5 * x[0] - x[0] * x[1], x[0] * x[1] - 3.0 * x[1]]   # noqa: E731
    target = solve_ivp(f, (0.0, 3.5), [1.0, 1.0], t_eval=ts, method="DOP853", rtol=1e-10, atol=1e-12).y.T[:, None, :]
    chain = kanode.Chain(kanode.KDense(2, 10, 5), kanode.KDense(10, 2, 5))
    p0 = chain.setup(np.random.default_rng(0))[0].astype(np.float64) / 1e5 * 1e4
    rhs = kanode.ChainRHS(chain, device=dev)
    u0 = np.array([[1.0, 1.0]])
    kw = dict(eta=1e-3, sensealg="interpolating_adjoint")

    def cpu(O, p):
        specs = [O.LayerSpec(2, 10, 5, "tanh_fast"), O.LayerSpec(10, 2, 5, "tanh_fast")]
        return O.chain_epoch(specs, p, u0, 3.5, ts, target, eta=1e-3)[2]
    return rhs, u0, (0.0, 3.5), ts, target, p0, kw, cpu, "device_adjoint"


def fk_problem(kanode, dev):
    from scipy.integrate import solve_ivp
    sys.path.insert(0, ROOT)
    import bench
    nx, dx, D, T = 26, 0.04, 0.01, 5.0
    x = np.arange(nx) * dx
    rho0 = (np.tanh((x - 0.4) / 0.02) - np.tanh((x - 0.6) / 0.02)) / 2
    lap = (np.diag(-2.0 * np.ones(nx)) + np.diag(np.ones(nx - 1), 1) + np.diag(np.ones(nx - 1), -1)) / dx ** 2
    lap[0, -1] = lap[-1, 0] = 1.0 / dx ** 2
    saveat = [0.5 * i for i in range(11)]
    truth = solve_ivp(lambda t, u: D * lap @ u + u * (1 - u), (0.0, T), rho0, t_eval=saveat, method="DOP853",
                      rtol=1e-10, atol=1e-12).y.T[:, None, :]
    kan1 = kanode.Chain(kanode.KDense(1, 1, 10, normalizer="softsign", basis_func="rbf"))
    rhs = kanode.FisherKPPRHS(kan1, nx=nx, dx=dx, D=D, dtype=torch.float64, device=dev)
    kw = dict(eta=1e-2)

    def cpu(O, p):
        return O.fk_fsens_epoch(O.LayerSpec(1, 1, 10, "softsign"), p, D, dx, rho0[None, :], T, saveat, truth, eta=1e-2)[2]
    return rhs, rho0[None, :], (0.0, T), saveat, truth, bench.fk_trained_like_params(), kw, cpu, "device_forward"


def stats(xs):
    med = float(np.median(xs))
    return {"median": med, "min": float(np.min(xs)), "max": float(np.max(xs)),
            "spread": float((np.max(xs) - np.min(xs)) / med)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--problems", default="lv,fk")
    ap.add_argument("--replicas", default="1,16,64,256,512")
    ap.add_argument("--iters", type=int, default=16, help="iterations per launch")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--legs", default="ens,seq")
    ap.add_argument("--no-cpu", action="store_true")
    ap.add_argument("--pkg", default=os.path.join(ROOT, "kan-odes_amd"), help="directory of the kanode package")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.rounds < 7:
        ap.error("--rounds must be at least 7 (the figure is a median, its spread the margin)")
    sys.path.insert(0, os.path.abspath(a.pkg))
    import kanode
    legs, K = a.legs.split(","), a.iters
    dev = torch.device("cuda:0")
    cus = torch.cuda.get_device_properties(dev).multi_processor_count
    out = {"unit": "ms per call of `iters` iterations", "iters": K, "rounds": a.rounds, "compute_units": cus,
           "pkg": os.path.relpath(os.path.dirname(kanode.LIB_PATH), ROOT)}
    for name in a.problems.split(","):
        rhs, u0_np, tspan, saveat, tgt_np, p0, kw, cpu, want = (lv_problem if name == "lv" else fk_problem)(kanode, dev)
        u0, tgt = torch.as_tensor(u0_np, device=dev), torch.as_tensor(tgt_np, device=dev)
        res = {}
        for R in [int(x) for x in a.replicas.split(",")]:
            p0s = torch.as_tensor(np.stack([p0 * (1.0 + 1e-4 * r) for r in range(R)]), device=dev)

            def leg(which):
                """One round from fresh trainers: (seconds, the loop that ran)."""
                if which == "ens":
                    ens = kanode.EnsembleTrainer(rhs, u0, tspan, saveat, tgt, p0s, **kw)
                    go = lambda: ens.run(K, chunk=K)                                   # noqa: E731
                else:
                    trs = [kanode.Trainer(rhs, u0, tspan, saveat, tgt, p0s[r], **kw) for r in range(R)]
                    go = lambda: [tr.run(K, chunk=K) for tr in trs]                    # noqa: E731
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                go()
                torch.cuda.synchronize()
                dt = time.perf_counter() - t0
                return dt, (ens.last_run if which == "ens" else trs[0].last_run)
            for which in legs:                             # warm-up: module load, buffers
                leg(which)
            times, path = {w: [] for w in legs}, {}
            for _ in range(a.rounds):
                for which in legs:
                    dt, path[which] = leg(which)
                    times[which].append(dt * 1e3)
            row = {}
            for which in legs:
                assert path[which] == want, (name, which, path[which])
                row[which] = stats(times[which])
                row[which]["replica_iters_per_s"] = R * K / (row[which]["median"] * 1e-3)
            if "ens" in row and "seq" in row:
                row["ens_over_seq"] = row["ens"]["median"] / row["seq"]["median"]
            res[str(R)] = row
        if not a.no_cpu:
            sys.path.insert(0, ROOT)
            from oracle import oracle as O
            pc, tc = p0.copy(), []
            for r in range(23):
                t0 = time.perf_counter()
                pc = cpu(O, pc)
                if r >= 3:
                    tc.append(time.perf_counter() - t0)
            ms = float(np.median(tc)) * 1e3
            res["cpu_one_core_ms_per_iteration"] = ms
            for R, row in ((k, v) for k, v in res.items() if k.isdigit()):
                row["cpu_16_cores_ms"] = -(-int(R) // 16) * K * ms          # ceil(R / 16) rounds of K iterations
                if "ens" in row:
                    row["ens_beats_16_cores"] = bool(row["ens"]["median"] < row["cpu_16_cores_ms"])
        out[name] = res
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
