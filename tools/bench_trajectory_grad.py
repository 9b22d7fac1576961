#!/usr/bin/env python
"""The gradient of a trajectory ensemble (kanode.trajectories_mse_gradient: R initial conditions of one problem, each
an ODE of its own with its own forward and adjoint step control, one workgroup each, one launch plus two reduction
launches) on tools/bench_trajectories.py's problem: the Lotka-Volterra KAN [2,10,2], G = 5, at the trained parameters
tests/golden/lv_trained_p_seed1.npy, from the first R of 4096 initial conditions default_rng(1).uniform(0.5, 2.0,
(4096, 2)), span (0, 3.5), saveat 0:0.1:3.4, default tolerances, fp64, against default_rng(5).uniform(0.5, 2,
(35, 4096, 2)).

Every leg is a wall-clock time around calls that end in a device synchronise; the legs run in turn round after round
(interleaved) after a warm-up of each; a leg's figure is the median over the rounds and its spread (max - min)/median
the margin any comparison is read against:
  grad<R>       one trajectories_mse_gradient call on the first R rows (--sizes)
  grad<R>cap<C> the same with the handle's fused_solve_cap = C (--caps): a smaller dense-output capacity, less LDS per
                workgroup, more workgroups per compute unit
  loop          native_mse_gradient at batch 1 for the first `--sample` rows: what a build without the entry offers
                for these semantics (a forward launch, an adjoint launch and host waits per trajectory).  SCALED by
                R / sample for each size, not run in full
  batched       Trainer.loss_and_grad() at the matrix u0 of 4096 rows: A DIFFERENT PROBLEM (ONE ODE over all entries,
                one step size); here for scale, not as a comparison
  train_any     one Trainer(device_loop="any").run(16) on a [2,4,2] chain   } code this entry does not change: the
  traj          one solve_trajectories call on the 4096 rows               } ratio to an older build's is a control
--legs loop,batched,train_any,traj uses only API an older build has (--pkg DIR: the directory holding that build's
`kanode` package).  The spread of the forward / adjoint step counts over the trajectories is recorded beside the times.
Prints one JSON line; --out writes it to a file as well.

    python tools/bench_trajectory_grad.py [--sizes 64,256,1024,4096] [--caps 64] [--sample 64] [--rounds 11]
                                          [--legs grad,loop,batched,train_any,traj] [--pkg DIR] [--out FILE]
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


def spread_of(xs):
    xs = np.asarray(xs)
    return {"min": int(xs.min()), "median": float(np.median(xs)), "max": int(xs.max()), "mean": float(xs.mean())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="64,256,1024,4096")
    ap.add_argument("--caps", default="", help="fused_solve_cap values for extra legs at the largest size")
    ap.add_argument("--sample", type=int, default=64, help="rows of the batch-1 loop that are run")
    ap.add_argument("--rounds", type=int, default=11)
    ap.add_argument("--legs", default="grad,loop,batched,train_any,traj")
    ap.add_argument("--pkg", default=os.path.join(ROOT, "kan-odes_amd"), help="directory of the kanode package")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.rounds < 10:
        ap.error("--rounds must be at least 10 (the figure is a median, its spread the margin)")
    sys.path.insert(0, os.path.abspath(a.pkg))
    import kanode
    from kanode.adjoint import native_mse_gradient
    if not torch.cuda.is_available():
        sys.exit("bench_trajectory_grad needs a GPU: a time taken elsewhere says nothing")
    dev = torch.device("cuda:0")
    want = a.legs.split(",")
    sizes = [int(s) for s in a.sizes.split(",")]
    caps = [int(c) for c in a.caps.split(",") if c]
    N_ALL, S = 4096, a.sample
    ts = [0.1 * i for i in range(35)]
    tspan = (0.0, 3.5)
    opt = kanode.Tsit5Options()
    u0 = torch.as_tensor(np.random.default_rng(1).uniform(0.5, 2.0, (N_ALL, 2)), device=dev).contiguous()
    X = torch.as_tensor(np.random.default_rng(5).uniform(0.5, 2, (35, N_ALL, 2)), device=dev).contiguous()
    p = torch.as_tensor(np.load(os.path.join(ROOT, "tests", "golden", "lv_trained_p_seed1.npy")).astype(np.float64),
                        device=dev)
    rhs = kanode.ChainRHS(kanode.Chain(kanode.KDense(2, 10, 5), kanode.KDense(10, 2, 5)), dtype=torch.float64,
                          device=dev)
    rows = [(u0[r:r + 1].contiguous(), X[:, r:r + 1].contiguous()) for r in range(S)]
    sub = {R: (u0[:R].contiguous(), X[:, :R].contiguous()) for R in sizes}
    # the [2,4,2] chain of tests/test_gpu_train_wg.py (shape S1) for the unchanged training loop
    s1 = kanode.ChainRHS(kanode.Chain(kanode.KDense(2, 4, 5), kanode.KDense(4, 2, 5)), dtype=torch.float64, device=dev)
    rng = np.random.default_rng(11)
    s1p = torch.as_tensor(rng.uniform(-0.3, 0.3, s1.hd.P), device=dev)
    s1u = torch.as_tensor(rng.uniform(0.5, 2.0, (1, 2)), device=dev)
    s1x = torch.as_tensor(rng.uniform(0.5, 2.0, (35, 1, 2)), device=dev)
    legs, res = [], {}
    if "grad" in want:
        legs += [f"grad{R}" for R in sizes] + [f"grad{sizes[-1]}cap{c}" for c in caps]
    legs += [w for w in ("loop", "batched", "train_any", "traj") if w in want]

    def leg(which):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        if which.startswith("grad"):
            R, _, cap = which[4:].partition("cap")
            u, x = sub[int(R)]
            if cap:
                with rhs.hd.options(fused_solve_cap=int(cap)):
                    out = kanode.trajectories_mse_gradient(rhs, u, tspan, p, ts, x, opt)
            else:
                out = kanode.trajectories_mse_gradient(rhs, u, tspan, p, ts, x, opt)
            assert out[2]["path"] == "device", which
            res[which] = out
        elif which == "loop":
            res["loop"] = [native_mse_gradient(rhs, u, tspan, p, ts, opt, x) for u, x in rows]
        elif which == "batched":
            tr = kanode.Trainer(rhs, u0, tspan, ts, X, p, solver=opt)
            res["batched"] = tr.loss_and_grad()
        elif which == "train_any":
            tr = kanode.Trainer(s1, s1u, tspan, ts, s1x, s1p, eta=1e-3, solver=opt, device_loop="any")
            tr.run(16)
            assert tr.last_run == "device_adjoint"
        else:
            res["traj"] = kanode.solve_trajectories(rhs, u0, tspan, p, ts, opt)
        torch.cuda.synchronize()
        return time.perf_counter() - t0
    for which in legs:                             # warm-up: module load, buffers
        leg(which)
    times = {w: [] for w in legs}
    for _ in range(a.rounds):
        for which in legs:
            times[which].append(leg(which) * 1e3)
    out = {"unit": "ms", "rounds": a.rounds, "sample": S,
           "compute_units": torch.cuda.get_device_properties(dev).multi_processor_count,
           "pkg": os.path.relpath(os.path.dirname(kanode.LIB_PATH), ROOT),
           "what": "LV KAN [2,10,2] G=5 at the trained parameters, fp64, tspan (0, 3.5), saveat 0:0.1:3.4, default "
                   "tolerances; loop = batch-1 native_mse_gradient on the first `sample` rows, scaled by R / sample"}
    for which in legs:
        out[which] = stats(times[which])
    if "loop" in legs:
        out["loop"]["us_per_gradient"] = out["loop"]["median"] * 1e3 / S
        out["loop"]["scaled_to"] = {str(R): out["loop"]["median"] * R / S for R in sizes}
    for which in legs:
        if not which.startswith("grad"):
            continue
        R = int(which[4:].partition("cap")[0])
        loss, dp, info = res[which]
        row = out[which]
        row["us_per_trajectory"] = row["median"] * 1e3 / R
        row["stopped"] = sum(s != "ok" for s in info["stop"])
        row["forward_iterations"] = spread_of([s["naccept"] + s["nreject"] for s in info["fwd_stats"]])
        row["adjoint_iterations"] = spread_of([s["naccept"] + s["nreject"] for s in info["adj_stats"]])
        row["group"] = rhs.hd.trajectories_gradient_group(0.0, 3.5, 35, opt.to_c())
        if "loop" in legs:
            row["over_scaled_loop"] = row["median"] / out["loop"]["scaled_to"][str(R)]
            if R >= S and "cap" not in which:   # the sampled rows are the call's first rows
                _, _, inf = kanode.trajectories_mse_gradient(rhs, sub[R][0], tspan, p, ts, sub[R][1], opt, rows=True)
                err = max(((inf["dp_rows"][r] - one[1]).abs().max() / one[1].abs().max()).item()
                          for r, one in enumerate(res["loop"]))
                row["max_rel_row_difference_to_loop_on_sample"] = err
    if "batched" in legs:
        out["batched"]["stats"] = {k: v for k, v in res["batched"][2].stats.items() if k in ("naccept", "nreject")}
        out["batched"]["note"] = "a different problem: ONE ODE over all entries, one step size"
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
