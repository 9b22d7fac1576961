#!/usr/bin/env python
"""ms per LV_driver_KANODE.jl iteration (:279-291) of one Lotka-Volterra trajectory, three ways in one process.

The problem is bench.py's lv1_train_bench (same p0, target, test problem, eta = 1e-3):
  run        Trainer.run at chunk = 256 with the test solve (the device-resident loop, kanode_train_tsit5)
  run_notest the same without the test solve
  step_loop  lv1_train_bench's loop: step() + eval_loss() + the (0, 14) test solve
  cpu        the C port on one core (O.chain_epoch + two O.chain_solve), median of 20 after 3 warm-ups
Prints one JSON line.  The number Trainer.run is judged against is `cpu` from the same run.

    python tools/bench_lv1_train.py [--iters 1024] [--chunk 256] [--reps 30] [--no-cpu]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "kan-odes_amd")]

import kanode  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=1024)
    ap.add_argument("--chunk", type=int, default=256)
    ap.add_argument("--reps", type=int, default=30, help="iterations of the step() loop")
    ap.add_argument("--no-cpu", action="store_true")
    a = ap.parse_args()
    from scipy.integrate import solve_ivp
    dev = torch.device("cuda:0")
    ts = [0.1 * i for i in range(35)]
    ts_test = [0.1 * i for i in range(141)]
    f = lambda t, x: [1.5 * x[0] - x[0] * x[1], x[0] * x[1] - 3.0 * x[1]]   # noqa: E731
    full = solve_ivp(f, (0.0, 14.0), [1.0, 1.0], t_eval=ts_test, method="DOP853", rtol=1e-10,
                     atol=1e-12).y.T[:, None, :]
    target = full[:35]
    chain = kanode.Chain(kanode.KDense(2, 10, 5), kanode.KDense(10, 2, 5))
    p0 = chain.setup(np.random.default_rng(0))[0].astype(np.float64) / 1e5 * 1e4
    rhs = kanode.ChainRHS(chain, device=dev)
    u0 = torch.tensor([[1.0, 1.0]], dtype=torch.float64, device=dev)
    tgt_test = torch.as_tensor(full, device=dev)

    def trainer():
        return kanode.Trainer(rhs, u0, (0.0, 3.5), ts, torch.as_tensor(target, device=dev),
                              torch.as_tensor(p0, device=dev), eta=1e-3, sensealg="interpolating_adjoint")

    out = {"unit": "ms/iteration", "iters": a.iters, "chunk": a.chunk,
           "native": bool(rhs.hd.train_supported(1))}
    test = ((0.0, 14.0), ts_test, tgt_test)
    for key, tst in (("run", test), ("run_notest", None)):
        tr = trainer()
        tr.run(min(a.chunk, 32), test=tst, chunk=a.chunk)          # warm-up: module load, buffers
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = tr.run(a.iters, test=tst, chunk=a.chunk)
        torch.cuda.synchronize()
        out[key] = (time.perf_counter() - t0) / a.iters * 1e3
        out[key + "_last_loss"] = float(r["loss"][-1])

    tr = trainer()

    def iteration():
        tr.step()
        tr.eval_loss()
        with torch.no_grad():
            return float(kanode.mse_loss(kanode.solve(rhs, u0, (0.0, 14.0), tr.p, ts_test).u, tgt_test))

    iteration()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(a.reps):
        iteration()
    torch.cuda.synchronize()
    out["step_loop"] = (time.perf_counter() - t0) / a.reps * 1e3
    if not a.no_cpu:
        from oracle import oracle as O
        specs = [O.LayerSpec(2, 10, 5, "tanh_fast"), O.LayerSpec(10, 2, 5, "tanh_fast")]
        u0c = np.array([[1.0, 1.0]])
        pc = p0.copy()
        times = []
        for r in range(23):
            t0 = time.perf_counter()
            _, _, pc, _, _ = O.chain_epoch(specs, pc, u0c, 3.5, ts, target, eta=1e-3)
            O.chain_solve(specs, pc, u0c, 3.5, ts)
            O.chain_solve(specs, pc, u0c, 14.0, ts_test)
            if r >= 3:
                times.append(time.perf_counter() - t0)
        out["cpu"] = float(np.median(times)) * 1e3
        out["run_over_cpu"] = out["run"] / out["cpu"]
    out["step_loop_over_run"] = out["step_loop"] / out["run"]
    print(json.dumps(out))


if __name__ == "__main__":
    main()
