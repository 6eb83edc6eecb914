#!/usr/bin/env python3
"""Exhaustive enumeration of RAND cases: every traitor message and every coin outcome
(docs/SEMANTICS.md §14), and the k_renum kernel's rate.

Sweep (default): for (n, m) and each f in --f, one representative faulty set per class
with f traitors (a class is: commander faulty or not, number of faulty lieutenants;
relabelling the lieutenants is a symmetry of the protocol, and the representative takes
the lowest indices), for the coins in --coins, the orders in --orders and R = 1, 2, ...
up to the largest that fits --max-bits (or the R of --phases).  Cases above --max-bits
(and above the library's 48) are listed as skipped.  The whole space 2^B is walked
through Engine.run_renum_device in calls of --chunk strategies; every call is
synchronised and timed on its own, and a call that took longer than --call-limit
seconds, or a case that has used --case-budget seconds, ends the case there: its line
then says how far it got ("complete": false).  One JSON line per case: B, strategies,
the counters, the IC1/IC2 witness, the stats (unsafe, undecided, decided_in, the two
witnesses and their decoded plays), seconds and strategies per second.

These limits are checked when a call has returned: they cannot end a launch that never
returns.  That bound has to come from outside the process: run the tool under
`timeout -k`, sized to the cases asked for.

    timeout -k 10 300 python tools/renum_sweep.py --n 4 --m 1 --f 1 --max-bits 34

--time: k_renum at (7, 2), R = 1, F = {1, 2}, local coins (35 bits), order attack, 2^30
strategies, counters and stats only, against two yardsticks: k_kenum KING3 at (7, 1),
F = {3} over 2^30 strategies (the same frame, one more round per phase, no D / V), and
k_rand BA_KING_SPLIT at (7, 2), R = 1 over 2^20 staged GIVEN trials with the same F.
The three alternate run by run; each run is one launch timed by the library's own HIP
events (ba_profile_enable); the lines give every run, the median, and the ratios of
k_renum's time per strategy-phase to k_kenum's per strategy-phase and to k_rand's per
trial-phase.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "byzantine-agreement_amd"))

from enum_common import run_case as walk, time_alternating  # noqa: E402

COINS = {"local": 0, "common": 1}


def classes(n, f):
    """[(F_0, faulty lieutenants, mask)] with f traitors in all."""
    out = []
    for f0 in (0, 1):
        fl = f - f0
        if 0 <= fl <= n - 1:
            out.append((f0, fl, f0 | (((1 << fl) - 1) << 1)))
    return out


def decoded(L, coin, n, m, R, F, S):
    """decode_rstrategy with JSON keys: "q:j>i" for a message, "p:g" / "p" for a toss."""
    if S is None:
        return None
    d = L.decode_rstrategy(coin, n, m, R, F, S)
    return {"messages": {f"{q}:{j}>{i}": v for (q, j, i), v in sorted(d["messages"].items())},
            "coins": {f"{p}" if g is None else f"{p}:{g}": v
                      for (p, g), v in sorted(d["coins"].items(), key=lambda kv: (kv[0][0], kv[0][1] or 0))}}


def run_case(eng, L, torch, coin, n, m, R, F, o, args):
    def call(first, count, d_cnt, d_wit, stream, d_stats):
        eng.run_renum_device(L.make_params(n, m, first_trial=first), coin, R, F, o, count, d_counters=d_cnt,
                             d_witness=d_wit, d_stats=d_stats, stream=stream)

    def stats_row(words):
        st = L.renum_stats(words)
        st["decided_in"] = st["decided_in"][:R + 1]
        return {"stats": st, "unsafe_play": decoded(L, coin, n, m, R, F, st["unsafe_witness"]),
                "undecided_play": decoded(L, coin, n, m, R, F, st["undecided_witness"])}

    head = {"coin": "common" if coin else "local", "n": n, "m": m, "phases": R, "faulty_mask": F, "order": o}
    return walk(call, L, torch, head, L.renum_bits(coin, n, m, R, F), args,
                stats=(L.RENUM_NSTATS, (2, 3), stats_row))


def sweep(args):
    import torch
    from ba_amd import lib as L
    eng = L.Engine(args.device)
    try:
        eng.run_renum(0, 4, 1, 1, 0b0010, 1)  # warm-up: module load
        cap = min(args.max_bits, L.ENUM_MAX_BITS)
        for f in args.f:
            for f0, fl, F in classes(args.n, f):
                for cname in args.coins:
                    coin = COINS[cname]
                    for R in (args.phases or range(1, L.RENUM_MAX_PHASES + 1)):
                        B = L.renum_bits(coin, args.n, args.m, R, F)
                        tag = dict(f=f, commander_faulty=f0, faulty_lieutenants=fl)
                        if B > cap:
                            print(json.dumps({"coin": cname, "n": args.n, "m": args.m, "phases": R,
                                              "faulty_mask": F, "bits": B, "skipped": f"more than {cap} bits",
                                              **tag}), flush=True)
                            if not args.phases:
                                break  # a larger R is larger still
                            continue
                        for o in args.orders:
                            row = run_case(eng, L, torch, coin, args.n, args.m, R, F, o, args)
                            row.update(tag)
                            print(json.dumps(row), flush=True)
    finally:
        eng.close()


def time_renum(args):
    import torch
    from ba_amd import lib as L
    n, o, S, T = 7, 1, 1 << 30, 1 << 20
    Fr, Fk = 0b0000110, 0b0001000
    assert L.renum_bits(0, n, 2, 1, Fr) == 35 and L.kenum_bits(1, n, 1, Fk) == 36
    Pk = L.king3_phases(n, 1)
    eng = L.Engine(args.device)
    try:
        s = torch.cuda.current_stream().cuda_stream
        fm = torch.full((T,), Fr, dtype=torch.int32, device="cuda")
        oc = torch.full((T,), o, dtype=torch.uint8, device="cuda")
        cnt = torch.zeros(16, dtype=torch.int64, device="cuda")
        wit = torch.full((1,), -1, dtype=torch.int64, device="cuda")
        sts = torch.zeros(L.RENUM_NSTATS, dtype=torch.int64, device="cuda")
        sts[2:4] = -1
        pr, pk = L.make_params(n, 2), L.make_params(n, 1)

        def renum():
            eng.run_renum_device(pr, 0, 1, Fr, o, S, d_counters=cnt.data_ptr(), d_witness=wit.data_ptr(),
                                 d_stats=sts.data_ptr(), stream=s)

        def kenum():
            eng.run_kenum_device(pk, 1, Fk, o, S, d_counters=cnt.data_ptr(), d_witness=wit.data_ptr(), stream=s)

        def rand():
            eng.run_rand_device(pr, T, 1, L.KING_SPLIT, L.RAND_LOCAL, d_faulty=fm.data_ptr(),
                                d_order=oc.data_ptr(), d_counters=cnt.data_ptr(), stream=s)

        # (kernel, what, fn, trials, phases, m, faulty mask)
        kernels = (("k_renum", "local coins, R = 1", renum, S, 1, 2, Fr),
                   ("k_kenum", "KING3", kenum, S, Pk, 1, Fk),
                   ("k_rand", "split, local coins, R = 1, staged GIVEN inputs", rand, T, 1, 2, Fr))
        ms = time_alternating(eng, torch, [(k[0], k[0], k[2]) for k in kernels], args.repeats)
        per = {}
        for name, what, _, count, phases, m, F in kernels:
            med = statistics.median(ms[name])
            per[name] = med * 1e-3 / (count * phases)
            print(json.dumps({"kernel": f"{name} {what}", "n": n, "m": m, "faulty_mask": F, "order": o,
                              "trials": count, "phases": phases, "outputs": "off",
                              "runs_ms": [round(x, 4) for x in ms[name]], "median_ms": round(med, 4),
                              "trials_per_s": float(f"{count / (med * 1e-3):.4e}"),
                              "seconds_per_trial_phase": float(f"{per[name]:.4e}")}), flush=True)
        print(json.dumps({"ratio": "k_renum seconds per strategy-phase / k_kenum KING3 seconds per strategy-phase",
                          "value": float(f"{per['k_renum'] / per['k_kenum']:.4e}")}), flush=True)
        print(json.dumps({"ratio": "k_renum seconds per strategy-phase / k_rand seconds per trial-phase",
                          "value": float(f"{per['k_renum'] / per['k_rand']:.4e}")}), flush=True)
    finally:
        eng.close()


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--n", type=int, default=4)
    ap.add_argument("--m", type=int, default=1)
    ap.add_argument("--f", type=int, nargs="+", default=[1])
    ap.add_argument("--coins", choices=sorted(COINS), nargs="+", default=["local", "common"])
    ap.add_argument("--orders", type=int, nargs="+", default=[0, 1])
    ap.add_argument("--phases", type=int, nargs="+", default=None,
                    help="the R to walk (default: 1, 2, ... while the case fits --max-bits)")
    ap.add_argument("--chunk", type=lambda v: int(v, 0), default=1 << 34,
                    help="strategies per device call (a multiple of 64)")
    ap.add_argument("--call-limit", type=float, default=30.0, help="seconds one call may take")
    ap.add_argument("--case-budget", type=float, default=120.0, help="seconds one case may take")
    ap.add_argument("--max-bits", type=int, default=40)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--time", action="store_true",
                    help="time k_renum against k_kenum and k_rand instead of sweeping")
    ap.add_argument("--repeats", type=int, default=7)
    args = ap.parse_args()
    (time_renum if args.time else sweep)(args)


if __name__ == "__main__":
    main()
