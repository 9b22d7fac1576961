#!/usr/bin/env python
"""ms per iteration of training a small chain that is not one Lotka-Volterra trajectory, legs interleaved.

Two cases: a pruned LV network [2,4,2] at one trajectory, and the LV network [2,10,2] on 16 initial conditions
(tanh_fast, G = 5, saveat 0:0.1:3.4 over (0, 3.5), default tolerances, eta = 1e-3; p0, u0 and the target from
default_rng(11), the target a DOP853 solution of the Lotka-Volterra equations from each u0).  Each round runs every
leg once for --iters iterations, in turn; the figure of a leg is the median over the rounds:
  run_any    Trainer(device_loop="any").run   (kd_chain_train_wg_kernel, kanode_train_tsit5)
  run        Trainer.run with the default device_loop (on these shapes: the host loop of step())
  step       a loop of Trainer.step() on the same handle
  cport      oracle.chain_epoch, the C port on one core, chained through its own Adam step
--legs run,step runs those alone: they use only API an older build has, so the same script measures them there
(--pkg DIR: the directory holding that build's `kanode` package, its libkanode.so inside).  Prints one JSON line;
--out writes it to a file as well.

    python tools/bench_train_any.py [--iters 64] [--rounds 7] [--legs run_any,run,step,cport] [--pkg DIR] [--out FILE]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = {"pruned_2_4_2_B1": ([2, 4, 2], 1), "lv_2_10_2_B16": ([2, 10, 2], 16)}
TS = [0.1 * i for i in range(35)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=64)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--legs", default="run_any,run,step,cport")
    ap.add_argument("--pkg", default=os.path.join(ROOT, "kan-odes_amd"), help="directory of the kanode package")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    sys.path.insert(0, os.path.abspath(a.pkg))
    sys.path.insert(0, ROOT)
    import kanode
    if a.rounds < 5:
        ap.error("--rounds must be at least 5 (the figure is a median)")
    legs = a.legs.split(",")
    from scipy.integrate import solve_ivp
    dev = torch.device("cuda:0")
    out = {"unit": "ms/iteration", "iters": a.iters, "rounds": a.rounds,
           "pkg": os.path.relpath(os.path.dirname(kanode.LIB_PATH), ROOT), "cases": {}}
    f = lambda t, x: [1.5 * x[0] - x[0] * x[1], x[0] * x[1] - 3.0 * x[1]]   # noqa: E731
    for cname, (w, B) in CASES.items():
        rng = np.random.default_rng(11)
        chain = kanode.Chain(*[kanode.KDense(i, o, 5) for i, o in zip(w, w[1:])])
        p0 = rng.uniform(-0.3, 0.3, chain.parameterlength())
        u0n = rng.uniform(0.5, 2.0, (B, 2))
        tgn = np.stack([solve_ivp(f, (0.0, 3.5), u0n[b], t_eval=TS, method="DOP853", rtol=1e-10, atol=1e-12).y.T
                        for b in range(B)], axis=1)
        rhs = kanode.ChainRHS(chain, device=dev)
        u0, tgt = torch.as_tensor(u0n, device=dev), torch.as_tensor(tgn, device=dev)

        def trainer(**kw):
            return kanode.Trainer(rhs, u0, (0.0, 3.5), TS, tgt, torch.as_tensor(p0, device=dev), eta=1e-3,
                                  sensealg="interpolating_adjoint", **kw)

        def leg(name):
            """One round of a leg from a fresh start: (seconds, last loss, the loop that ran)."""
            if name == "cport":
                from oracle import oracle as O
                specs = [O.LayerSpec(i, o, 5, "tanh_fast") for i, o in zip(w, w[1:])]
                p, secs = p0.copy(), 0.0
                for _ in range(a.iters):          # (its Adam has no moments carried over: timing only)
                    last, _, p, _, s = O.chain_epoch(specs, p, u0n, 3.5, TS, tgn, eta=1e-3)
                    secs += s
                return secs, last, "c_port"
            tr = trainer(device_loop="any") if name == "run_any" else trainer()
            if name != "run_any" and "train_any_chain" in kanode._lib.OPTIONS:
                rhs.hd.set_option("train_any_chain", 0)   # (run_any turned it on, on the shared handle)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            if name == "step":
                for _ in range(a.iters):
                    last = tr.step()
                how = "step"
            else:
                last = float(tr.run(a.iters, chunk=a.iters)["loss"][-1])
                how = tr.last_run
            torch.cuda.synchronize()
            return time.perf_counter() - t0, last, how

        for name in legs:                              # warm-up: module load, buffers
            leg(name)
        times = {name: [] for name in legs}
        info = {}
        for _ in range(a.rounds):
            for name in legs:
                dt, last, how = leg(name)
                times[name].append(dt / a.iters * 1e3)
                info[name] = (last, how)
        c = {"chain": w, "batch": B, "P": int(chain.parameterlength())}
        for name in legs:
            c[name] = float(np.median(times[name]))
            c[name + "_min"] = float(np.min(times[name]))
            c[name + "_max"] = float(np.max(times[name]))
            c[name + "_last_loss"], c[name + "_path"] = info[name]
        if "run_any" in c and "step" in c:
            c["step_over_run_any"] = c["step"] / c["run_any"]
        out["cases"][cname] = c
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
