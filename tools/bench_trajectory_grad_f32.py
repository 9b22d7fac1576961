#!/usr/bin/env python
"""The gradient of a trajectory ensemble on an fp32 handle (kanode.trajectories_mse_gradient(f32="device"):
kanode_trajectories_gradient_f32_tsit5, one one-wave workgroup per trajectory, one launch plus two reduction launches),
the sibling of tools/bench_trajectory_grad.py on the same problem cast to float32: the Lotka-Volterra KAN [2,10,2],
G = 5, at the trained parameters tests/golden/lv_trained_p_seed1.npy, from the first R of 4096 initial conditions
default_rng(1).uniform(0.5, 2.0, (4096, 2)), span (0, 3.5), saveat 0:0.1:3.4, default tolerances, against
default_rng(5).uniform(0.5, 2, (35, 4096, 2)).

Every leg is a wall-clock time around calls that end in a device synchronise; the legs run in turn round after round
(interleaved) after a warm-up of each; a leg's figure is the median over the rounds and its spread (max - min)/median
the margin any comparison is read against:
  f32grad<R>        one trajectories_mse_gradient(f32="device") call on the first R rows of the fp32 problem (--sizes)
  f32grad<R>cap<C>  the same with the handle's fused_solve_cap = C (--caps)
  f64grad<R>        the fp64 entry on the fp64 problem at the same sizes
  f32loop           native_mse_gradient at batch 1 on the fp32 handle for the first `--sample` rows: what a build
                    without the fp32 entry offers for these semantics.  SCALED by R / sample for each size
  f32traj           one solve_trajectories call on the 4096 fp32 rows    } code the fp32 entry does not change: the
  train_any         one Trainer(device_loop="any").run(16), [2,4,2] fp64 } ratio to an older build's is a control
--legs f64grad,f32loop,f32traj,train_any uses only API the parent build has (--pkg DIR: the directory holding that
build's `kanode` package).  Prints one JSON line; --out writes it to a file as well.

    python tools/bench_trajectory_grad_f32.py [--sizes 64,256,1024,4096] [--caps 64,128] [--sample 64] [--rounds 11]
                                              [--legs f32grad,f64grad,f32loop,f32traj,train_any] [--pkg DIR]
                                              [--out FILE]
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
from bench_trajectory_grad import spread_of   # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="64,256,1024,4096")
    ap.add_argument("--caps", default="", help="fused_solve_cap values for extra fp32 legs at the largest size")
    ap.add_argument("--sample", type=int, default=64, help="rows of the batch-1 loop that are run")
    ap.add_argument("--rounds", type=int, default=11)
    ap.add_argument("--legs", default="f32grad,f64grad,f32loop,f32traj,train_any")
    ap.add_argument("--pkg", default=os.path.join(ROOT, "kan-odes_amd"), help="directory of the kanode package")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.rounds < 10:
        ap.error("--rounds must be at least 10 (the figure is a median, its spread the margin)")
    sys.path.insert(0, os.path.abspath(a.pkg))
    import kanode
    from kanode.adjoint import native_mse_gradient
    if not torch.cuda.is_available():
        sys.exit("bench_trajectory_grad_f32 needs a GPU: a time taken elsewhere says nothing")
    dev = torch.device("cuda:0")
    want = a.legs.split(",")
    sizes = [int(s) for s in a.sizes.split(",")]
    caps = [int(c) for c in a.caps.split(",") if c]
    N_ALL, S = 4096, a.sample
    ts = [0.1 * i for i in range(35)]
    tspan = (0.0, 3.5)
    opt = kanode.Tsit5Options()
    u0 = np.random.default_rng(1).uniform(0.5, 2.0, (N_ALL, 2))
    X = np.random.default_rng(5).uniform(0.5, 2, (35, N_ALL, 2))
    p = np.load(os.path.join(ROOT, "tests", "golden", "lv_trained_p_seed1.npy")).astype(np.float64)
    prob = {}
    for dt in (torch.float32, torch.float64):
        rhs = kanode.ChainRHS(kanode.Chain(kanode.KDense(2, 10, 5), kanode.KDense(10, 2, 5)), dtype=dt, device=dev)
        u, x = (torch.as_tensor(v, dtype=dt, device=dev).contiguous() for v in (u0, X))
        prob[dt] = dict(rhs=rhs, p=torch.as_tensor(p, dtype=dt, device=dev), u0=u, X=x,
                        sub={R: (u[:R].contiguous(), x[:, :R].contiguous()) for R in sizes},
                        rows=[(u[r:r + 1].contiguous(), x[:, r:r + 1].contiguous()) for r in range(S)])
    f32, f64 = prob[torch.float32], prob[torch.float64]
    # the [2,4,2] chain of tests/test_gpu_train_wg.py (shape S1) for the unchanged training loop
    s1 = kanode.ChainRHS(kanode.Chain(kanode.KDense(2, 4, 5), kanode.KDense(4, 2, 5)), dtype=torch.float64, device=dev)
    rng = np.random.default_rng(11)
    s1p = torch.as_tensor(rng.uniform(-0.3, 0.3, s1.hd.P), device=dev)
    s1u = torch.as_tensor(rng.uniform(0.5, 2.0, (1, 2)), device=dev)
    s1x = torch.as_tensor(rng.uniform(0.5, 2.0, (35, 1, 2)), device=dev)
    legs, res = [], {}
    if "f32grad" in want:
        legs += [f"f32grad{R}" for R in sizes] + [f"f32grad{sizes[-1]}cap{c}" for c in caps]
    if "f64grad" in want:
        legs += [f"f64grad{R}" for R in sizes]
    legs += [w for w in ("f32loop", "f32traj", "train_any") if w in want]

    def leg(which):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        if which.startswith(("f32grad", "f64grad")):
            q = f32 if which.startswith("f32") else f64
            kw = {"f32": "device"} if q is f32 else {}
            R, _, cap = which[7:].partition("cap")
            u, x = q["sub"][int(R)]
            if cap:
                with q["rhs"].hd.options(fused_solve_cap=int(cap)):
                    out = kanode.trajectories_mse_gradient(q["rhs"], u, tspan, q["p"], ts, x, opt, **kw)
            else:
                out = kanode.trajectories_mse_gradient(q["rhs"], u, tspan, q["p"], ts, x, opt, **kw)
            assert out[2]["path"] == "device", which
            res[which] = out
        elif which == "f32loop":
            res[which] = [native_mse_gradient(f32["rhs"], u, tspan, f32["p"], ts, opt, x) for u, x in f32["rows"]]
        elif which == "f32traj":
            res[which] = kanode.solve_trajectories(f32["rhs"], f32["u0"], tspan, f32["p"], ts, opt)
        else:
            tr = kanode.Trainer(s1, s1u, tspan, ts, s1x, s1p, eta=1e-3, solver=opt, device_loop="any")
            tr.run(16)
            assert tr.last_run == "device_adjoint"
        torch.cuda.synchronize()
        return time.perf_counter() - t0
    for which in legs:                             # warm-up: module load, buffers
        leg(which)
    times = {w: [] for w in legs}
    for _ in range(a.rounds):
        for which in legs:
            times[which].append(leg(which) * 1e3)
    cus = torch.cuda.get_device_properties(dev).multi_processor_count
    out = {"unit": "ms", "rounds": a.rounds, "sample": S, "compute_units": cus,
           "pkg": os.path.relpath(os.path.dirname(kanode.LIB_PATH), ROOT),
           "what": "LV KAN [2,10,2] G=5 at the trained parameters, tspan (0, 3.5), saveat 0:0.1:3.4, default "
                   "tolerances; f32* on the float32 problem, f64* on the float64 one; f32loop = batch-1 "
                   "native_mse_gradient on the first `sample` fp32 rows, scaled by R / sample"}
    for which in legs:
        out[which] = stats(times[which])
    if "f32loop" in legs:
        out["f32loop"]["us_per_gradient"] = out["f32loop"]["median"] * 1e3 / S
        out["f32loop"]["scaled_to"] = {str(R): out["f32loop"]["median"] * R / S for R in sizes}
    for which in legs:
        if not which.startswith(("f32grad", "f64grad")):
            continue
        q = f32 if which.startswith("f32") else f64
        R = int(which[7:].partition("cap")[0])
        loss, dp, info = res[which]
        row = out[which]
        row["us_per_trajectory"] = row["median"] * 1e3 / R
        row["stopped"] = sum(s != "ok" for s in info["stop"])
        row["forward_iterations"] = spread_of([s["naccept"] + s["nreject"] for s in info["fwd_stats"]])
        row["adjoint_iterations"] = spread_of([s["naccept"] + s["nreject"] for s in info["adj_stats"]])
        hd = q["rhs"].hd
        row["group"] = (hd.trajectories_gradient_f32_group if q is f32 else hd.trajectories_gradient_group)(
            0.0, 3.5, 35, opt.to_c())
        if q is f32 and "f32loop" in legs:
            row["over_scaled_loop"] = row["median"] / out["f32loop"]["scaled_to"][str(R)]
        twin = "f64grad" + which[7:]
        if q is f32 and twin in legs:
            row["over_f64"] = row["median"] / out[twin]["median"]
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
