#!/usr/bin/env python
"""ms per Trainer.loss_and_grad() on fields of 65 to 128 entries, forward mode against the adjoint, in one process.

Shapes (Nx, B) = (26, 3) and (89, 1) at G = 10 (tests/fsens_restatement.py's initial conditions and parameters) on
the reference horizon: T = 5, saveat 0.5, the default tolerances.  Per shape:
  forward   sensealg = "auto": ForwardDiffSensitivity by the two-entries-per-lane one-workgroup solve
            (kanode_forward_sensitivity_tsit5 with KANODE_OPT_FSENS_WIDE, turned on by the host rule)
  adjoint   sensealg = "interpolating_adjoint" on the same build: what these shapes ran before the option existed
  cpu       oracle.fk_fsens_epoch (the C Dual solve + Adam) on one core
The two GPU arms run in interleaved rounds; medians (and minima) over the rounds.  Prints one JSON line.

    python tools/bench_fsens_wide.py [--rounds 30] [--no-cpu]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "kan-odes_amd"), os.path.join(ROOT, "tests")]

import kanode  # noqa: E402
import fsens_restatement as R  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=30)
    ap.add_argument("--no-cpu", action="store_true")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    T, saveat = 5.0, [0.5 * i for i in range(11)]
    out = {"unit": "ms per loss_and_grad", "rounds": a.rounds, "T": T, "shapes": {}}
    for Nx, B in ((26, 3), (89, 1)):
        pr = R.problem(Nx, B, 10)
        kan1 = kanode.Chain(kanode.KDense(1, 1, 10, normalizer="softsign"))
        p = torch.as_tensor(pr["p"], device=dev)
        u0 = torch.as_tensor(pr["u0"], device=dev)
        import bench
        truth_p = torch.as_tensor(bench.fk_trained_like_params(), device=dev)
        arms, res = {}, {}
        for name, sa in (("forward", None), ("adjoint", "interpolating_adjoint")):
            rhs = kanode.FisherKPPRHS(kan1, nx=Nx, dx=pr["dx"], D=pr["D"], device=dev)
            with torch.no_grad():
                X = kanode.solve(rhs, u0, (0.0, T), truth_p, saveat).u
            arms[name] = kanode.Trainer(rhs, u0, (0.0, T), saveat, X, p, eta=1e-2, sensealg=sa)
        times = {k: [] for k in arms}
        for r in range(a.rounds + 3):
            for name, tr in arms.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                loss, g, sol = tr.loss_and_grad()
                float(loss)
                torch.cuda.synchronize()
                if r >= 3:
                    times[name].append(time.perf_counter() - t0)
                if r == 0:
                    res[name + "_path"] = sol.stats.get("sensealg", "interpolating_adjoint")
                    res[name + "_naccept"] = int(sol.stats.get("naccept", -1))
                    res[name + "_grad"] = g.cpu().numpy()
        for name in arms:
            res[name] = float(np.median(times[name])) * 1e3
            res[name + "_min"] = float(np.min(times[name])) * 1e3
        gf, ga = res.pop("forward_grad"), res.pop("adjoint_grad")
        res["grad_rel_diff"] = float(np.abs(gf - ga).max() / np.abs(ga).max())
        if not a.no_cpu:
            Xc = arms["forward"].target.cpu().numpy()
            ts = []
            for r in range(13):
                _, _, _, st, secs = R.O.fk_fsens_epoch(pr["spec"], pr["p"], pr["D"], pr["dx"], pr["u0"], T, saveat, Xc,
                                                        eta=1e-2)
                if r >= 3:
                    ts.append(secs)
            res["cpu"] = float(np.median(ts)) * 1e3
            res["cpu_naccept"] = st["naccept"]
            res["forward_over_cpu"] = res["forward"] / res["cpu"]
        res["forward_over_adjoint"] = res["forward"] / res["adjoint"]
        out["shapes"][f"{Nx}x{B}"] = res
    print(json.dumps(out))


if __name__ == "__main__":
    main()
