#!/usr/bin/env python3
"""Randomized agreement (Ben-Or rounds, docs/SEMANTICS.md §13) beside OM(m) and KING3
over the fault fraction, and k_rand's time per launch.

Sweep (default): for one (n, m) run f = 0..n traitors (FAULTY_EXACT, random orders)
through Engine.run (OM(m), where its tree is admitted), Engine.run_king3 under both
policies and Engine.run_rand with the local and the common coin under both policies,
--phases phases, on the same seed -- all see the same faulty sets and orders -- and
print one JSON line per f: each protocol's rates (king_sweep's), and for every RAND
variant the counters, the histogram of `decided`, its mean over the decided trials and
the shares of 255 (undecided within R) and 254 (unsafe).

    python tools/rand_sweep.py --n 10 --m 3 --trials 65536 --phases 32

--time: 1,048,576 trials per launch on staged inputs at every --time-shape, k_rand with
--time-phases phases (both coins, both policies) beside k_king3 COIN and SPLIT, the
launches alternating (enum_common.time_alternating), each timed by the library's own
HIP events; median, minimum and maximum over --repeats runs.  Two staged input sets:
"exact" has f = m traitors in every trial, so every word is in bound and k_rand's early
finish can fire; "mixed" is FAULTY_RANDOM with f = n, which puts an out-of-bound trial
into every word (the share of such words is printed), so every word runs all its
phases.  Beside each time: the distinct Philox calls per word when every sender is
faulty in the word (ba_rand_coin_calls / ba_king3_coin_calls), the calls a wave issues
for them when it runs every phase and draws every toss (a call is issued for all 64
lanes), and the time the bare Philox stream needs for the issued calls at
--philox-rate calls/s.
"""
from __future__ import annotations

import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "byzantine-agreement_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

from enum_common import time_alternating  # noqa: E402
from king_sweep import rates  # noqa: E402


def decided_stats(L, np, decided):
    hist = np.bincount(decided, minlength=256)
    done = decided[decided < L.RAND_UNSAFE]
    return {"decided_hist": {str(p): int(c) for p, c in enumerate(hist[:L.RAND_UNSAFE]) if c},
            "mean_decided_phase": float(done.mean()) if len(done) else None,
            "undecided": float(hist[L.RAND_UNDECIDED] / len(decided)),
            "unsafe": float(hist[L.RAND_UNSAFE] / len(decided))}


def wave_calls(n, phases, coin_policy, king3):
    """Philox calls one wave issues per word when every sender is faulty somewhere in
    the word, every phase runs and (k_rand) every toss is drawn: the commander's send,
    per all-to-all round one call per group member (groups of up to four sender pairs
    per lane), and per phase the king's send (k_king3) or the toss (k_rand)."""
    npairs = (n + 1) // 2
    per_round = sum(min(4, (npairs - v0 + 1) // 2) for v0 in range(0, npairs, 8))
    if king3:
        return 1 + phases * (2 * per_round + 1) if coin_policy else 0
    return (1 + phases * 2 * per_round if coin_policy else 0) + phases


def sweep(args):
    import numpy as np
    from ba_amd import lib as L
    eng = L.Engine(args.device)
    try:
        for f in range(args.n + 1):
            kw = dict(seed=args.seed, faulty_mode=L.FAULTY_EXACT, f=f, order_mode=L.ORDER_RANDOM,
                      want_decisions=False, want_outcome=False)
            row = {"n": args.n, "m": args.m, "f": f, "trials": args.trials, "phases": args.phases,
                   "king3_phases": L.king3_phases(args.n, args.m)}
            try:
                row["om"] = rates(eng.run(args.n, args.m, args.trials, **kw).counters)
            except L.BAError as e:  # the relay tree is too large, or m > 8
                row["om"] = None
                row["om_error"] = e.code
            for pname, pol in (("coin", L.KING_COIN), ("split", L.KING_SPLIT)):
                r = eng.run_king3(args.n, args.m, args.trials, pol, want_settled=True, **kw)
                row["king3_" + pname] = rates(r.counters)
                row["king3_" + pname]["unsettled"] = float(np.mean(r.settled == L.KING_UNSETTLED))
                for cname, coin in (("local", L.RAND_LOCAL), ("common", L.RAND_COMMON)):
                    r = eng.run_rand(args.n, args.m, args.trials, args.phases, pol, coin,
                                     want_decided=True, **kw)
                    row[f"rand_{cname}_{pname}"] = {**rates(r.counters), "counters": r.counters,
                                                    **decided_stats(L, np, r.decided)}
            print(json.dumps(row), flush=True)
    finally:
        eng.close()


def time_rand(args):
    import numpy as np
    import torch
    from ba_amd import lib as L
    T, R = args.time_trials, args.time_phases
    words = (T + 63) // 64
    eng = L.Engine(args.device)
    try:
        s = torch.cuda.current_stream().cuda_stream
        dec = torch.empty(T, dtype=torch.int64, device="cuda")
        out = torch.empty(T, dtype=torch.uint8, device="cuda")
        dcd = torch.empty(T, dtype=torch.uint8, device="cuda")
        cnt = torch.zeros(16, dtype=torch.int64, device="cuda")
        for n, m in args.time_shape:
            ins = {}
            for name, mode, f in (("exact", L.FAULTY_EXACT, m), ("mixed", L.FAULTY_RANDOM, n)):
                fm = torch.empty(T, dtype=torch.int32, device="cuda")
                oc = torch.empty(T, dtype=torch.uint8, device="cuda")
                # the inputs do not depend on m, and ba_gen_inputs_device admits m <= 8 only
                eng.gen_inputs_device(L.make_params(n, min(m, 8), seed=args.seed, faulty_mode=mode, f=f,
                                                    order_mode=L.ORDER_RANDOM), T,
                                      d_faulty=fm.data_ptr(), d_order=oc.data_ptr(), stream=s)
                torch.cuda.synchronize()
                nf = np.unpackbits(fm.cpu().numpy().view(np.uint8)).reshape(-1, 32).sum(axis=1)
                oob = (nf[:T // 64 * 64].reshape(-1, 64) > m).any(axis=1)
                ins[name] = (fm, oc, float(oob.mean()))
            p = L.make_params(n, m, seed=args.seed)

            def io(name):
                fm, oc, _ = ins[name]
                return dict(d_faulty=fm.data_ptr(), d_order=oc.data_ptr(), d_decisions=dec.data_ptr(),
                            d_outcome=out.data_ptr(), d_counters=cnt.data_ptr(), stream=s)

            kernels, meta = [], {}
            for pname, pol in (("COIN", L.KING_COIN), ("SPLIT", L.KING_SPLIT)):
                key = f"k_king3/{pname}"
                kernels.append((key, "k_king3", lambda pol=pol: eng.run_king3_device(p, T, pol, **io("exact"))))
                meta[key] = {"inputs": "exact", "phases": L.king3_phases(n, m),
                             "coin_calls_per_word": L.king3_coin_calls(n, m) if pname == "COIN" else 0,
                             "wave_calls": wave_calls(n, L.king3_phases(n, m), pname == "COIN", True)}
                for cname, coin in (("LOCAL", L.RAND_LOCAL), ("COMMON", L.RAND_COMMON)):
                    # the `decided` output (its per-phase checks) is timed at COIN / COMMON only
                    for inp, want in (("exact", False), ("mixed", False), ("exact", True), ("mixed", True)):
                        if want and (pname, cname) != ("COIN", "COMMON"):
                            continue
                        key = f"k_rand/{pname}/{cname}/{inp}" + ("/decided" if want else "")
                        kernels.append((key, "k_rand", lambda pol=pol, coin=coin, inp=inp, want=want:
                                        eng.run_rand_device(p, T, R, pol, coin,
                                                            d_decided=dcd.data_ptr() if want else 0, **io(inp))))
                        tosses = R * (n if coin == L.RAND_LOCAL else 1)
                        meta[key] = {"inputs": inp, "phases": R, "decided_output": want,
                                     "coin_calls_per_word": L.rand_coin_calls(n, R, coin) if pname == "COIN"
                                     else tosses,
                                     "wave_calls": wave_calls(n, R, pname == "COIN", False)}
            ms = time_alternating(eng, torch, kernels, args.repeats)
            for key, _, _ in kernels:
                v = sorted(ms[key])
                med = v[len(v) // 2] * 1e3
                calls = meta[key].pop("wave_calls")
                bound = calls * 64 * words / args.philox_rate * 1e6
                print(json.dumps({"kernel": key, "n": n, "m": m, "trials_per_launch": T, "runs": len(v),
                                  **meta[key], "words_with_out_of_bound_trial": ins[meta[key]["inputs"]][2],
                                  "median_us_per_launch": round(med, 2), "min_us_per_launch": round(v[0] * 1e3, 2),
                                  "max_us_per_launch": round(v[-1] * 1e3, 2),
                                  "us_per_phase": round(med / meta[key]["phases"], 2),
                                  "issued_wave_calls_per_word_full_run": calls,
                                  "philox_calls_per_s": args.philox_rate,
                                  "bound_philox_us_full_run": round(bound, 2),
                                  "philox_share_of_time_full_run": round(bound / med, 4) if med else None}),
                      flush=True)
    finally:
        eng.close()


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--n", type=int, default=10)
    ap.add_argument("--m", type=int, default=3)
    ap.add_argument("--trials", type=int, default=65536)
    ap.add_argument("--phases", type=int, default=32, help="R of the sweep")
    ap.add_argument("--seed", type=int, default=0xBA5EED)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--time", action="store_true", help="time k_rand beside k_king3 instead of sweeping")
    ap.add_argument("--time-shape", type=lambda v: tuple(int(x, 0) for x in v.split(",")), nargs="+",
                    default=[(10, 3), (32, 10)], metavar="N,M")
    ap.add_argument("--time-trials", type=int, default=1 << 20)
    ap.add_argument("--time-phases", type=int, default=16, help="R of the timed launches")
    ap.add_argument("--repeats", type=int, default=31)
    ap.add_argument("--philox-rate", type=float, default=1.055e12,
                    help="bare Philox stream, calls/s (profiles/r14a_king3_time.jsonl, 4 waves/SIMD)")
    args = ap.parse_args()
    (time_rand if args.time else sweep)(args)


if __name__ == "__main__":
    main()
