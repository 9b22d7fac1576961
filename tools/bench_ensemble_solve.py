#!/usr/bin/env python
"""Replica-solves per second of the ensemble solve (kanode.solve_ensemble: R parameter vectors of one problem, one
workgroup each, one launch) against R kanode.solve calls one after another, on two problems:
  lv   the Lotka-Volterra test solve of tools/bench_lv1_train.py: span (0, 14), saveat 0.1
  fk   the Fisher-KPP field (26, 1, G = 10) of tools/bench_fk26_train.py: T = 5, saveat 0.5
Replica r solves at p0·(1 + 1e-4·r).

For every R of --replicas the two legs run in turn, round after round (interleaved), after a warm-up call of each:
  ens   one solve_ensemble call                 one launch of R workgroups (two for fk: the R tables first)
  seq   R solve calls, one after another        R launches of one workgroup, R host waits
A leg's figure is the median over the rounds, and its spread (max - min)/median over those rounds is the margin any
comparison between legs is read against.

--legs seq uses only API an older build has, so the same script times the sequential leg there
(--pkg DIR: the directory holding that build's `kanode` package, its libkanode.so inside): that is the baseline.
Prints one JSON line; --out writes it to a file as well.

    python tools/bench_ensemble_solve.py [--problems lv,fk] [--replicas 1,16,64,256,512,1024] [--rounds 7]
                                         [--legs ens,seq] [--pkg DIR] [--out FILE]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bench_ensemble import fk_problem, lv_problem, stats   # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--problems", default="lv,fk")
    ap.add_argument("--replicas", default="1,16,64,256,512,1024")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--legs", default="ens,seq")
    ap.add_argument("--pkg", default=os.path.join(ROOT, "kan-odes_amd"), help="directory of the kanode package")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.rounds < 7:
        ap.error("--rounds must be at least 7 (the figure is a median, its spread the margin)")
    sys.path.insert(0, os.path.abspath(a.pkg))
    import kanode
    legs = a.legs.split(",")
    dev = torch.device("cuda:0")
    cus = torch.cuda.get_device_properties(dev).multi_processor_count
    out = {"unit": "ms per call (ens) / per R calls (seq)", "rounds": a.rounds, "compute_units": cus,
           "pkg": os.path.relpath(os.path.dirname(kanode.LIB_PATH), ROOT)}
    opt = kanode.Tsit5Options()
    for name in a.problems.split(","):
        rhs, u0_np, tspan, saveat, _, p0, _, _, _ = (lv_problem if name == "lv" else fk_problem)(kanode, dev)
        if name == "lv":   # the test problem of the training driver: four times the training span
            tspan, saveat = (0.0, 14.0), [0.1 * i for i in range(141)]
        u0 = torch.as_tensor(u0_np, device=dev)
        res = {}
        for R in [int(x) for x in a.replicas.split(",")]:
            ps = torch.as_tensor(np.stack([p0 * (1.0 + 1e-4 * r) for r in range(R)]), device=dev)
            rows = [ps[r].contiguous() for r in range(R)]

            def leg(which):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                if which == "ens":
                    sol = kanode.solve_ensemble(rhs, u0, tspan, ps, saveat, opt)
                    assert sol.path == "device" and sol.stop == ["ok"] * R, (name, R, sol.path)
                else:
                    for r in range(R):
                        kanode.solve(rhs, u0, tspan, rows[r], saveat, opt)
                torch.cuda.synchronize()
                return time.perf_counter() - t0
            for which in legs:                             # warm-up: module load, buffers
                leg(which)
            times = {w: [] for w in legs}
            for _ in range(a.rounds):
                for which in legs:
                    times[which].append(leg(which) * 1e3)
            row = {}
            for which in legs:
                row[which] = stats(times[which])
                row[which]["replica_solves_per_s"] = R / (row[which]["median"] * 1e-3)
            if "ens" in row and "seq" in row:
                row["ens_over_seq"] = row["ens"]["median"] / row["seq"]["median"]
            res[str(R)] = row
        out[name] = res
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
