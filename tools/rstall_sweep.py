#!/usr/bin/env python3
"""RAND against the stalling adversary (docs/SEMANTICS.md §15) beside RAND's two sampled
adversaries, over the fault count and both coins.

For one (n, m) run f = 0..n traitors (FAULTY_EXACT, random orders) through
Engine.run_rstall and through Engine.run_rand under BA_KING_COIN and BA_KING_SPLIT, with
the local and the common coin, at every --phases R, on the same seed -- all see the same
faulty sets and orders -- and print one JSON line per (R, f): for each adversary and
coin the mean and the last phase by which every loyal general had decided, the share of
trials undecided within R (255) and the share unsafe (254).  k_rand takes up to 64
phases: beyond, its columns are absent.

    python tools/rstall_sweep.py --n 10 --m 3 --trials 65536 --phases 64 250
"""
from __future__ import annotations

import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "byzantine-agreement_amd"))


def columns(L, np, res):
    hist = np.bincount(res.decided, minlength=256)
    done = res.decided[res.decided < L.RAND_UNSAFE]
    return {"mean_decided_phase": round(float(done.mean()), 4) if len(done) else None,
            "last_decided_phase": int(done.max()) if len(done) else None,
            "undecided": float(hist[L.RAND_UNDECIDED] / len(res.decided)),
            "unsafe": float(hist[L.RAND_UNSAFE] / len(res.decided)),
            "bound_violations": res.counters["bound_violations"], "in_bound": res.counters["in_bound"]}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--n", type=int, default=10)
    ap.add_argument("--m", type=int, default=3)
    ap.add_argument("--trials", type=int, default=65536)
    ap.add_argument("--phases", type=int, nargs="+", default=[64, 250], help="every R of the sweep")
    ap.add_argument("--seed", type=int, default=0xBA5EED)
    ap.add_argument("--device", type=int, default=0)
    args = ap.parse_args()
    import numpy as np
    from ba_amd import lib as L
    eng = L.Engine(args.device)
    try:
        for R in args.phases:
            for f in range(args.n + 1):
                kw = dict(seed=args.seed, faulty_mode=L.FAULTY_EXACT, f=f, order_mode=L.ORDER_RANDOM,
                          want_decisions=False, want_outcome=False, want_decided=True)
                row = {"n": args.n, "m": args.m, "f": f, "trials": args.trials, "phases": R}
                for cname, coin in (("local", L.RAND_LOCAL), ("common", L.RAND_COMMON)):
                    row[f"stall_{cname}"] = columns(L, np, eng.run_rstall(args.n, args.m, args.trials, R, coin, **kw))
                    if R <= L.RAND_MAX_PHASES:
                        for pname, pol in (("coin", L.KING_COIN), ("split", L.KING_SPLIT)):
                            row[f"{pname}_{cname}"] = columns(
                                L, np, eng.run_rand(args.n, args.m, args.trials, R, pol, coin, **kw))
                print(json.dumps(row), flush=True)
    finally:
        eng.close()


if __name__ == "__main__":
    main()
