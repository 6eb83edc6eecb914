#!/usr/bin/env python3
"""Exhaustive traitor-strategy enumeration of OM(m) cases (docs/SEMANTICS.md §8), and the
k_enum kernel's rate.

Sweep (default): for (n, m) and each f in --f, one representative faulty set per class
([F_0], f_L) with F_0 + f_L = f -- the commander or not, and the lowest f_L lieutenants;
all 12 counters depend on F through the class only -- whose space has at most 48 bits,
for the orders retreat and attack.  The whole space 2^B is walked through
Engine.run_enum_device in calls of --chunk strategies; every call is synchronised and
timed on its own, and a call that took longer than --call-limit seconds, or a case that
has used --case-budget seconds, ends the case there: its line then says how far it got
("complete": false).  One JSON line per case: B, strategies, the counters, the witness,
seconds and strategies per second.

These limits are checked when a call has returned: they keep a slow run short (a call is
2^34 strategies, 0.05 s at the measured rate), they cannot end a launch that never
returns.  That bound has to come from outside the process: run the tool under
`timeout -k`, sized to the cases asked for, as the committed records were.

    timeout -k 10 700 python tools/enum_sweep.py --n 7 --m 2 --f 0 1 2

--time: k_enum against k_adv SPLIT (the yardstick: the same walk, but with per-trial
inputs and a per-trial epilogue) at (7, 2), F = {1}, order attack, 2^25 trials, both on
device buffers with the per-trial outputs off, k_adv on staged GIVEN inputs.  The two
alternate run by run; each run is one launch timed by the library's own HIP events
(ba_profile_enable); the line gives every run and the median.
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


def classes(n, f):
    """[(F_0, f_L, representative mask)] with F_0 + f_L = f."""
    out = []
    for f0 in (0, 1):
        fl = f - f0
        if 0 <= fl <= n - 1:
            out.append((f0, fl, f0 | (((1 << fl) - 1) << 1)))
    return out


def run_case(eng, L, torch, n, m, F, o, args):
    def call(first, count, d_cnt, d_wit, stream):
        eng.run_enum_device(L.make_params(n, m, first_trial=first), F, o, count, d_counters=d_cnt,
                            d_witness=d_wit, stream=stream)

    return walk(call, L, torch, {"n": n, "m": m, "faulty_mask": F, "order": o}, L.enum_bits(n, m, F), args)


def sweep(args):
    import torch
    from ba_amd import lib as L
    eng = L.Engine(args.device)
    try:
        eng.run_enum(4, 1, 0b0011, 1)  # warm-up: module load, scratch
        for f in args.f:
            for f0, fl, F in classes(args.n, f):
                B = L.enum_bits(args.n, args.m, F)
                if B > min(args.max_bits, L.ENUM_MAX_BITS):
                    print(json.dumps({"n": args.n, "m": args.m, "faulty_mask": F, "bits": B,
                                      "skipped": f"more than {min(args.max_bits, L.ENUM_MAX_BITS)} bits"}),
                          flush=True)
                    continue
                for o in args.orders:
                    row = run_case(eng, L, torch, args.n, args.m, F, o, args)
                    row.update(f=f, commander_faulty=f0, faulty_lieutenants=fl)
                    print(json.dumps(row), flush=True)
    finally:
        eng.close()


def time_enum(args):
    import torch
    from ba_amd import lib as L
    n, m, F, o, T = 7, 2, 0b0000010, 1, 1 << 25
    assert L.enum_bits(n, m, F) == 25
    eng = L.Engine(args.device)
    try:
        s = torch.cuda.current_stream().cuda_stream
        fm = torch.full((T,), F, dtype=torch.int32, device="cuda")
        oc = torch.full((T,), o, dtype=torch.uint8, device="cuda")
        cnt = torch.zeros(16, dtype=torch.int64, device="cuda")
        wit = torch.full((1,), -1, dtype=torch.int64, device="cuda")
        p = L.make_params(n, m)

        def enum():
            eng.run_enum_device(p, F, o, T, d_counters=cnt.data_ptr(), d_witness=wit.data_ptr(), stream=s)

        def adv():
            eng.run_adv_device(p, T, L.ADV_SPLIT, d_faulty=fm.data_ptr(), d_order=oc.data_ptr(),
                               d_counters=cnt.data_ptr(), stream=s)

        kernels = (("k_enum", "k_enum", enum), ("k_adv", "k_adv", adv))
        ms = time_alternating(eng, torch, kernels, args.repeats)
        for name, _, _ in kernels:
            med = statistics.median(ms[name])
            print(json.dumps({"kernel": name + (" split, staged GIVEN inputs" if name == "k_adv" else ""),
                              "n": n, "m": m, "faulty_mask": F, "order": o, "trials": T,
                              "outputs": "off", "runs_ms": [round(x, 4) for x in ms[name]],
                              "median_ms": round(med, 4),
                              "trials_per_s": float(f"{T / (med * 1e-3):.4e}")}), flush=True)
    finally:
        eng.close()


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--n", type=int, default=7)
    ap.add_argument("--m", type=int, default=2)
    ap.add_argument("--f", type=int, nargs="+", default=[0, 1, 2])
    ap.add_argument("--orders", type=int, nargs="+", default=[0, 1])
    ap.add_argument("--chunk", type=lambda v: int(v, 0), default=1 << 34,
                    help="strategies per device call (a multiple of 64)")
    ap.add_argument("--call-limit", type=float, default=30.0, help="seconds one call may take")
    ap.add_argument("--case-budget", type=float, default=300.0, help="seconds one case may take")
    ap.add_argument("--max-bits", type=int, default=48)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--time", action="store_true", help="time k_enum against k_adv instead of sweeping")
    ap.add_argument("--repeats", type=int, default=7)
    args = ap.parse_args()
    (time_enum if args.time else sweep)(args)


if __name__ == "__main__":
    main()
