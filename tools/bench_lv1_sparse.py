#!/usr/bin/env python
"""ms per iteration of the sparsified Lotka-Volterra training (the driver's sparse_on = 1), legs interleaved.

The problem is tools/bench_lv1_train.py's (bench.py's lv1_train_bench: same p0, target, eta = 1e-3), without the
test solve.  Each round runs every leg once for --iters iterations, in turn; the figure of a leg is the median
over the rounds:
  run_l0     Trainer.run, sparse_reg = 0        (the device-resident loop, kanode_train_tsit5)
  run_l1     Trainer.run, sparse_reg = 5e-4     (the same loop with the L1 term)
  step_l1    a loop of Trainer.step(), sparse_reg = 5e-4
--legs step_l1 runs that leg alone: it uses only API an older build has, so the same script measures it there
(--pkg DIR: the directory holding that build's `kanode` package, its libkanode.so inside).  Prints one JSON line;
--out writes it to a file as well.

    python tools/bench_lv1_sparse.py [--iters 128] [--rounds 7] [--legs run_l0,run_l1,step_l1] [--pkg DIR] [--out FILE]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LAM = 5e-4


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=128)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--legs", default="run_l0,run_l1,step_l1")
    ap.add_argument("--pkg", default=os.path.join(ROOT, "kan-odes_amd"), help="directory of the kanode package")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    sys.path.insert(0, os.path.abspath(a.pkg))
    import kanode
    if a.rounds < 5:
        ap.error("--rounds must be at least 5 (the figure is a median)")
    legs = a.legs.split(",")
    from scipy.integrate import solve_ivp
    dev = torch.device("cuda:0")
    ts = [0.1 * i for i in range(35)]
    f = lambda t, x: [1.5 * x[0] - x[0] * x[1], x[0] * x[1] - 3.0 * x[1]]   # noqa: E731
    target = solve_ivp(f, (0.0, 3.5), [1.0, 1.0], t_eval=ts, method="DOP853", rtol=1e-10, atol=1e-12).y.T[:, None, :]
    chain = kanode.Chain(kanode.KDense(2, 10, 5), kanode.KDense(10, 2, 5))
    p0 = chain.setup(np.random.default_rng(0))[0].astype(np.float64) / 1e5 * 1e4
    rhs = kanode.ChainRHS(chain, device=dev)
    u0 = torch.tensor([[1.0, 1.0]], dtype=torch.float64, device=dev)
    tgt = torch.as_tensor(target, device=dev)

    def trainer(lam):
        return kanode.Trainer(rhs, u0, (0.0, 3.5), ts, tgt, torch.as_tensor(p0, device=dev), eta=1e-3,
                              sensealg="interpolating_adjoint", sparse_reg=lam)

    def leg(name):
        """One round of a leg from a fresh trainer: (seconds, last loss, the loop run() took)."""
        tr = trainer(0.0 if name == "run_l0" else LAM)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        if name == "step_l1":
            for _ in range(a.iters):
                last = tr.step()
            how = "step"
        else:
            last = float(tr.run(a.iters, chunk=a.iters)["loss"][-1])
            how = tr.last_run
        torch.cuda.synchronize()
        return time.perf_counter() - t0, last, how

    for name in legs:                                  # warm-up: module load, buffers
        leg(name)
    times = {name: [] for name in legs}
    info = {}
    for _ in range(a.rounds):
        for name in legs:
            dt, last, how = leg(name)
            times[name].append(dt / a.iters * 1e3)
            info[name] = (last, how)
    out = {"unit": "ms/iteration", "iters": a.iters, "rounds": a.rounds, "lambda": LAM,
           "pkg": os.path.relpath(os.path.dirname(kanode.LIB_PATH), ROOT)}
    for name in legs:
        out[name] = float(np.median(times[name]))
        out[name + "_min"] = float(np.min(times[name]))
        out[name + "_max"] = float(np.max(times[name]))
        out[name + "_last_loss"], out[name + "_path"] = info[name]
    if "run_l0" in out and "run_l1" in out:
        out["run_l1_over_run_l0"] = out["run_l1"] / out["run_l0"]
    if "step_l1" in out and "run_l1" in out:
        out["step_l1_over_run_l1"] = out["step_l1"] / out["run_l1"]
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
