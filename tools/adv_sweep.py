#!/usr/bin/env python3
"""OM(m) against scripted traitors over the fault count, and the k_adv kernel's rate.

Sweep (default): for one (n, m) run f = 0..n traitors (FAULTY_EXACT, random orders)
through Engine.run (every traitor flips a fair coin) and Engine.run_adv for each
policy (SPLIT, FLIP, ANTI; docs/SEMANTICS.md §7) on the same seed -- all four see
the same faulty sets and orders -- and print one JSON line per f with each
adversary's agreement, validity and bound-violation rates.

    python tools/adv_sweep.py --n 4 --m 2 --trials 65536

--time: k_adv at n = 10, m = 3, 1,048,576 trials per launch (--time-shape: another
shape) through Engine.run_adv_device on staged inputs, one policy after another,
and Engine.run_device (the coin engine) on the same inputs in the same run, the
kernels alternating window by window.  Each window is timed with HIP events and
lasts at least --window seconds, after a warm-up window of the same length.  Every
figure printed is measured; nodes_per_word is computed from the shape.
"""
from __future__ import annotations

import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "byzantine-agreement_amd"))

POLICIES = (("split", 0), ("flip", 1), ("anti", 2))


def rates(c):
    t, appl = c["trials"], c["validity_applicable"]
    return {
        "agreement": c["agreement"] / t,
        "validity": c["validity"] / appl if appl else None,
        "in_bound": c["in_bound"] / t,
        "bound_violations": c["bound_violations"] / t,
        "undefined_decisions_per_trial": c["undefined_decisions"] / t,
    }


def sweep(args):
    from ba_amd import lib as L
    eng = L.Engine(args.device)
    try:
        for f in range(args.n + 1):
            kw = dict(seed=args.seed, faulty_mode=L.FAULTY_EXACT, f=f, order_mode=L.ORDER_RANDOM,
                      want_decisions=False, want_outcome=False)
            row = {"n": args.n, "m": args.m, "f": f, "trials": args.trials,
                   "coin": rates(eng.run(args.n, args.m, args.trials, **kw).counters)}
            for name, policy in POLICIES:
                row[name] = rates(eng.run_adv(args.n, args.m, args.trials, policy, **kw).counters)
            print(json.dumps(row), flush=True)
    finally:
        eng.close()


def walk_nodes(n, m):
    """Tree nodes the receivers of one 64-trial word visit: (n-1) sum_k P(n-2, k)."""
    L, me = n - 1, min(m, n - 2) if n >= 2 else 0
    per, p = 0, 1
    for k in range(me + 1):
        per += p
        p *= L - 1 - k
    return L * per


def time_adv(args):
    import torch
    from ba_amd import lib as L
    n, m, f, T = args.time_shape
    eng = L.Engine(args.device)
    try:
        kw = dict(seed=args.seed, faulty_mode=L.FAULTY_RANDOM, f=f, order_mode=L.ORDER_RANDOM)
        s = torch.cuda.current_stream().cuda_stream
        fm = torch.empty(T, dtype=torch.int32, device="cuda")
        oc = torch.empty(T, dtype=torch.uint8, device="cuda")
        dec = torch.empty(T, dtype=torch.int64, device="cuda")
        out = torch.empty(T, dtype=torch.uint8, device="cuda")
        cnt = torch.zeros(16, dtype=torch.int64, device="cuda")
        eng.gen_inputs_device(L.make_params(n, m, **kw), T, d_faulty=fm.data_ptr(), d_order=oc.data_ptr(),
                              stream=s)
        p = L.make_params(n, m, seed=args.seed)
        io = dict(d_faulty=fm.data_ptr(), d_order=oc.data_ptr(), d_decisions=dec.data_ptr(),
                  d_outcome=out.data_ptr(), d_counters=cnt.data_ptr(), stream=s)

        def launch(policy):
            if policy is None:
                eng.run_device(p, T, **io)
            else:
                eng.run_adv_device(p, T, policy, **io)

        def window(policy, k):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(k):
                launch(policy)
            e1.record()
            e1.synchronize()
            return e0.elapsed_time(e1) * 1e-3

        kernels = [("ba_run_trials_device", None)] + [("k_adv " + nm, pol) for nm, pol in POLICIES]
        count = {}
        for name, policy in kernels:  # warm-up, then launches per window
            window(policy, 20)
            per = window(policy, 50) / 50
            k = max(50, int(args.window / per * 1.1) + 1)
            while window(policy, k) < args.window:  # also the warm-up window at this length
                k = int(k * 1.3) + 1
            count[name] = k
        rows = {name: [] for name, _ in kernels}
        for _ in range(args.repeats):  # the kernels alternate window by window
            for name, policy in kernels:
                rows[name].append(window(policy, count[name]))
        torch.cuda.synchronize()
        L.check_handoff(cnt)
        for name, policy in kernels:
            k, sec = count[name], min(rows[name])
            print(json.dumps({
                "kernel": name, "n": n, "m": m, "f_max": f, "trials_per_launch": T, "inputs": "staged",
                "launches": k, "window_s": round(sec, 4), "windows_s": [round(r, 4) for r in rows[name]],
                "us_per_launch": round(sec / k * 1e6, 2),
                "trials_per_s": float(f"{k * T / sec:.4e}"),
                "nodes_per_word": walk_nodes(n, m) if policy is not None else None,
            }), flush=True)
    finally:
        eng.close()


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--n", type=int, default=4)
    ap.add_argument("--m", type=int, default=2)
    ap.add_argument("--trials", type=int, default=65536)
    ap.add_argument("--seed", type=int, default=0xBA5EED)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--time", action="store_true", help="time k_adv instead of sweeping")
    ap.add_argument("--time-shape", type=lambda v: tuple(int(x, 0) for x in v.split(",")),
                    default=(10, 3, 3, 1 << 20), metavar="N,M,F,TRIALS",
                    help="--time: another shape (f ~ U{0..F} traitors), e.g. 7,2,7,1048576")
    ap.add_argument("--window", type=float, default=0.5, help="seconds per timed window")
    ap.add_argument("--repeats", type=int, default=3)
    args = ap.parse_args()
    (time_adv if args.time else sweep)(args)


if __name__ == "__main__":
    main()
