#!/usr/bin/env python
"""The trajectory ensemble (kanode.solve_trajectories: R initial conditions of one problem, each an ODE of its own
with its own step control, a 16-lane row each, one launch) on bench.py's lv4096 problem: the Lotka-Volterra KAN
[2,10,2], G = 5, at the trained parameters tests/golden/lv_trained_p_seed1.npy, from 4096 initial conditions
default_rng(1).uniform(0.5, 2.0, (4096, 2)), span (0, 3.5), saveat 0:0.1:3.4, default tolerances; fp32 and fp64.

Three legs, each a wall-clock time around calls that end in a device synchronise, run in turn round after round
(interleaved) after a warm-up of each; a leg's figure is the median over the rounds and its spread
(max - min)/median the margin any comparison is read against:
  traj     one solve_trajectories call             one launch, R / 4 one-wave workgroups
  batched  one solve() of the matrix u0            A DIFFERENT PROBLEM: ONE ODE over all 2R entries, one error norm,
                                                   its own step count; here for scale, not as a comparison
  loop     solve() at batch 1 for `--sample` of    what a build without solve_trajectories offers for these semantics:
           the R rows, scaled by R / sample        R launches and R host waits.  SCALED from the sample, not run in
                                                   full (the rows are the first `sample` of u0)
--legs loop,batched uses only API an older build has (--pkg DIR: the directory holding that build's `kanode` package).
The spread of naccept / nreject over the R trajectories and the batched solve's counts are recorded beside the times.
Prints one JSON line; --out writes it to a file as well.

    python tools/bench_trajectories.py [--dtypes f32,f64] [--n 4096] [--sample 64] [--rounds 11]
                                       [--legs traj,batched,loop] [--pkg DIR] [--out FILE]
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
from bench_ensemble import stats   # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dtypes", default="f32,f64")
    ap.add_argument("--n", type=int, default=4096, help="initial conditions")
    ap.add_argument("--sample", type=int, default=64, help="rows of the batch-1 loop that are run")
    ap.add_argument("--rounds", type=int, default=11)
    ap.add_argument("--legs", default="traj,batched,loop")
    ap.add_argument("--pkg", default=os.path.join(ROOT, "kan-odes_amd"), help="directory of the kanode package")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.rounds < 10:
        ap.error("--rounds must be at least 10 (the figure is a median, its spread the margin)")
    sys.path.insert(0, os.path.abspath(a.pkg))
    import kanode
    legs = a.legs.split(",")
    if not torch.cuda.is_available():
        sys.exit("bench_trajectories needs a GPU: a time taken elsewhere says nothing")
    dev = torch.device("cuda:0")
    R, S = a.n, min(a.sample, a.n)
    ts = [0.1 * i for i in range(35)]
    tspan = (0.0, 3.5)
    u0n = np.random.default_rng(1).uniform(0.5, 2.0, (R, 2))
    p0 = np.load(os.path.join(ROOT, "tests", "golden", "lv_trained_p_seed1.npy"))
    opt = kanode.Tsit5Options()
    out = {"unit": "ms", "rounds": a.rounds, "n": R, "sample": S,
           "compute_units": torch.cuda.get_device_properties(dev).multi_processor_count,
           "pkg": os.path.relpath(os.path.dirname(kanode.LIB_PATH), ROOT),
           "what": "LV KAN [2,10,2] G=5 at the trained parameters, tspan (0, 3.5), saveat 0:0.1:3.4, default "
                   "tolerances; loop = batch-1 solve() on the first `sample` rows, scaled by n / sample"}
    for name in a.dtypes.split(","):
        dtype = {"f32": torch.float32, "f64": torch.float64}[name]
        chain = kanode.Chain(kanode.KDense(2, 10, 5), kanode.KDense(10, 2, 5))
        rhs = kanode.ChainRHS(chain, dtype=dtype, device=dev)
        u0 = torch.as_tensor(u0n, dtype=dtype, device=dev).contiguous()
        p = torch.as_tensor(p0, dtype=dtype, device=dev)
        rows = [u0[r:r + 1].contiguous() for r in range(S)]
        res = {}

        def leg(which):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            if which == "traj":
                sol = kanode.solve_trajectories(rhs, u0, tspan, p, ts, opt)
                assert sol.path == "device" and sol.stop == ["ok"] * R, (name, sol.path)
                res["sol"] = sol
            elif which == "batched":
                res["bat"] = kanode.solve(rhs, u0, tspan, p, ts, opt)
            else:
                res["loop"] = [kanode.solve(rhs, rows[r], tspan, p, ts, opt) for r in range(S)]
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
        if "loop" in row:
            row["loop"]["note"] = f"{S} batch-1 solves timed; scaled_to_n = median * n / sample"
            row["loop"]["scaled_to_n"] = row["loop"]["median"] * R / S
            row["loop"]["us_per_solve"] = row["loop"]["median"] * 1e3 / S
        if "traj" in row:
            sol = res["sol"]
            nacc = np.array([s["naccept"] for s in sol.stats])
            nrej = np.array([s["nreject"] for s in sol.stats])
            row["traj"]["us_per_trajectory"] = row["traj"]["median"] * 1e3 / R
            row["traj"]["naccept"] = {"min": int(nacc.min()), "median": float(np.median(nacc)),
                                      "max": int(nacc.max()), "mean": float(nacc.mean())}
            row["traj"]["nreject"] = {"min": int(nrej.min()), "median": float(np.median(nrej)),
                                      "max": int(nrej.max()), "with_rejections": int((nrej > 0).sum())}
            # a wave runs as long as the longest of its four rows
            its = (nacc + nrej)[:R - R % 4].reshape(-1, 4)
            if its.size:
                row["traj"]["iterations_wave_max_over_mean"] = float(its.max(axis=1).mean() / its.mean())
            if "loop" in res:   # the sampled rows are the launch's first rows: the same bits
                same = all(torch.equal(sol.u[:, r:r + 1, :], one.u) and sol.stats[r] == one.stats
                           for r, one in enumerate(res["loop"]))
                row["traj"]["equals_batch1_on_sample"] = bool(same)
        if "batched" in row:
            row["batched"]["stats"] = res["bat"].stats
            row["batched"]["note"] = "a different problem: ONE ODE over all entries, one step size"
        if "traj" in row and "loop" in row:
            row["traj_over_scaled_loop"] = row["traj"]["median"] / row["loop"]["scaled_to_n"]
        out[name] = row
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
