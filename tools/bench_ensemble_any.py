#!/usr/bin/env python
"""Ensemble training of the small chains that are not the Lotka-Volterra shape (kanode_fit_ensemble_tsit5:
EnsembleTrainer(device_loop="any"), R replicas, one workgroup each, one launch per group) against R
Trainer(device_loop="any").run calls one after another and against the C port, on two shapes:
  S1   a pruned [2,4,2] net on one trajectory           (the WideModel adjoint)
  S3   [2,7,2] on 16 initial conditions                 (four waves, a 1.8 MB private block at 1024 steps)
with the 35-row saveat list over (0, 3.5), random targets and the default solver options (adaptive steps).

For every R of --replicas the legs run in turn, round after round (interleaved), each from fresh trainers (replica r
starts from p0 scaled by 1 + 1e-4·r), --iters iterations in one launch per call:
  ens   EnsembleTrainer(device_loop="any").run(iters, chunk=iters)                one launch of R workgroups
  seq   R times Trainer(device_loop="any").run(iters, chunk=iters), in turn        R launches of one workgroup
  cpu   the C port on one core (oracle: chain_epoch), per iteration
A leg's figure is the median over the rounds, and its spread (max - min)/median over those rounds is the margin any
comparison between legs is read against.

--legs seq uses only API an older build has, so the same script times Trainer.run there (--pkg DIR: the directory
holding that build's `kanode` package, its libkanode.so inside); run the two builds in turn in one visit.
--cap N sets KANODE_OPT_FUSED_SOLVE_CAP (0: the library's rule): a smaller capacity needs less LDS.
Prints one JSON line; --out writes it to a file as well.

    python tools/bench_ensemble_any.py [--shapes S1,S3] [--replicas 1,16,64,256,512] [--iters 16] [--rounds 7]
                                       [--legs ens,seq,cpu] [--cap N] [--pkg DIR] [--out FILE]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = {"S1": ([2, 4, 2], 1), "S3": ([2, 7, 2], 16)}
TS = [0.1 * i for i in range(35)]


def problem(kanode, sid, dev):
    w, B = SHAPES[sid]
    chain = kanode.Chain(*[kanode.KDense(i, o, 5) for i, o in zip(w, w[1:])])
    rng = np.random.default_rng(11)
    p0 = rng.uniform(-0.3, 0.3, chain.parameterlength())
    u0 = rng.uniform(0.5, 2.0, (B, w[0]))
    X = rng.uniform(0.5, 2.0, (35, B, w[0]))
    return kanode.ChainRHS(chain, device=dev), p0, u0, X


def stats(xs):
    med = float(np.median(xs))
    return {"median": med, "min": float(np.min(xs)), "max": float(np.max(xs)),
            "spread": float((np.max(xs) - np.min(xs)) / med)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="S1,S3")
    ap.add_argument("--replicas", default="1,16,64,256,512")
    ap.add_argument("--iters", type=int, default=16, help="iterations per launch")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--legs", default="ens,seq,cpu")
    ap.add_argument("--cap", type=int, default=0, help="KANODE_OPT_FUSED_SOLVE_CAP (0: the library's rule)")
    ap.add_argument("--pkg", default=os.path.join(ROOT, "kan-odes_amd"), help="directory of the kanode package")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.rounds < 7:
        ap.error("--rounds must be at least 7 (the figure is a median, its spread the margin)")
    sys.path.insert(0, os.path.abspath(a.pkg))
    import kanode
    legs = [x for x in a.legs.split(",") if x != "cpu"]
    K = a.iters
    dev = torch.device("cuda:0")
    cus = torch.cuda.get_device_properties(dev).multi_processor_count
    out = {"unit": "ms per call of `iters` iterations", "iters": K, "rounds": a.rounds, "compute_units": cus,
           "fused_solve_cap": a.cap, "pkg": os.path.relpath(os.path.dirname(kanode.LIB_PATH), ROOT)}
    for sid in a.shapes.split(","):
        rhs, p0, u0_np, X_np = problem(kanode, sid, dev)
        if a.cap:
            rhs.hd.set_option("fused_solve_cap", a.cap)
        u0, tgt = torch.as_tensor(u0_np, device=dev), torch.as_tensor(X_np, device=dev)
        res = {}
        for R in [int(x) for x in a.replicas.split(",")] if legs else []:
            p0s = torch.as_tensor(np.stack([p0 * (1.0 + 1e-4 * r) for r in range(R)]), device=dev)

            def leg(which):
                """One round from fresh trainers: (seconds, the loop that ran)."""
                if which == "ens":
                    ens = kanode.EnsembleTrainer(rhs, u0, (0.0, 3.5), TS, tgt, p0s, eta=1e-3, device_loop="any")
                    go = lambda: ens.run(K, chunk=K)                                   # noqa: E731
                else:
                    trs = [kanode.Trainer(rhs, u0, (0.0, 3.5), TS, tgt, p0s[r], eta=1e-3, device_loop="any")
                           for r in range(R)]
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
                assert path[which] == "device_adjoint", (sid, which, path[which])
                row[which] = stats(times[which])
                row[which]["replica_iters_per_s"] = R * K / (row[which]["median"] * 1e-3)
            if "ens" in row and "seq" in row:
                row["ens_over_seq"] = row["ens"]["median"] / row["seq"]["median"]
            if "ens" in row:
                row["launch_group"] = rhs.hd.fit_ensemble_group(SHAPES[sid][1], 0.0, 3.5, len(TS), 0,
                                                                kanode.Tsit5Options().to_c())
            res[str(R)] = row
            print(sid, R, {w: round(row[w]["median"], 3) for w in legs}, file=sys.stderr, flush=True)
        if "cpu" in a.legs.split(","):
            sys.path.insert(0, ROOT)
            from oracle import oracle as O
            w, _ = SHAPES[sid]
            specs = [O.LayerSpec(i, o, 5, "tanh_fast") for i, o in zip(w, w[1:])]
            pc, tc = p0.copy(), []
            for r in range(23):
                t0 = time.perf_counter()
                pc = O.chain_epoch(specs, pc, u0_np, 3.5, TS, X_np, eta=1e-3)[2]
                if r >= 3:
                    tc.append(time.perf_counter() - t0)
            ms = float(np.median(tc)) * 1e3
            res["cpu_one_core_ms_per_iteration"] = ms
            for R, row in ((k, v) for k, v in res.items() if k.isdigit()):
                row["cpu_16_cores_ms"] = -(-int(R) // 16) * K * ms          # ceil(R / 16) rounds of K iterations
                if "ens" in row:
                    row["ens_beats_16_cores"] = bool(row["ens"]["median"] < row["cpu_16_cores_ms"])
        out[sid] = res
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
