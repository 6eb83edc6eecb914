#!/usr/bin/env python3
"""Exhaustive traitor-strategy enumeration of Phase King and KING3 cases
(docs/SEMANTICS.md §11), and the k_kenum kernel's rate.

Sweep (default): for (proto, n, m) and each f in --f, one representative faulty set per
class with f traitors, for the orders retreat and attack.  A class is (commander faulty
or not, faulty kings among the lieutenants 1..P-1, other faulty lieutenants);
relabelling the generals within a class is a symmetry of the protocol, and the
representative takes the lowest indices of each group.  Cases above --max-bits (and
above the library's 48) are listed as skipped.  The whole space 2^B is walked through
Engine.run_kenum_device in calls of --chunk strategies; every call is synchronised and
timed on its own, and a call that took longer than --call-limit seconds, or a case that
has used --case-budget seconds, ends the case there: its line then says how far it got
("complete": false).  One JSON line per case: B, strategies, the counters, the witness,
seconds and strategies per second.

These limits are checked when a call has returned: they cannot end a launch that never
returns.  That bound has to come from outside the process: run the tool under
`timeout -k`, sized to the cases asked for.

    timeout -k 10 300 python tools/kenum_sweep.py --proto king3 --n 4 --m 1 --f 1

--time: k_kenum KING3 at (7, 1), F = {3}, order attack, 2^30 strategies, counters only,
against k_king3 BA_KING_SPLIT (the yardstick: the same rounds, but with per-trial inputs,
LDS planes and a per-trial epilogue) at (7, 1) over 2^20 staged GIVEN trials with the
same F.  The two alternate run by run; each run is one launch timed by the library's own
HIP events (ba_profile_enable); the lines give every run, the median, and the ratio of
k_kenum's time per strategy to k_king3's time per trial.
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

PROTOS = {"king": 0, "king3": 1}


def classes(n, P, f):
    """[(F_0, faulty kings among the lieutenants, other faulty lieutenants, mask)] with f
    traitors in all; the kings are generals 0..P-1."""
    out = []
    for f0 in (0, 1):
        for fk in range(0, min(P - 1, n - 1) + 1):
            fo = f - f0 - fk
            if fo < 0 or fo > n - P:
                continue
            mask = f0 | (((1 << fk) - 1) << 1) | (((1 << fo) - 1) << P)
            out.append((f0, fk, fo, mask))
    return out


def run_case(eng, L, torch, proto, n, m, F, o, args):
    def call(first, count, d_cnt, d_wit, stream):
        eng.run_kenum_device(L.make_params(n, m, first_trial=first), proto, F, o, count, d_counters=d_cnt,
                             d_witness=d_wit, stream=stream)

    head = {"proto": args.proto, "n": n, "m": m, "faulty_mask": F, "order": o}
    return walk(call, L, torch, head, L.kenum_bits(proto, n, m, F), args)


def sweep(args):
    import torch
    from ba_amd import lib as L
    proto = PROTOS[args.proto]
    P = (L.king_phases if proto == 0 else L.king3_phases)(args.n, args.m)
    eng = L.Engine(args.device)
    try:
        eng.run_kenum(0, 4, 1, 0b0010, 1)  # warm-up: module load
        cap = min(args.max_bits, L.ENUM_MAX_BITS)
        for f in args.f:
            for f0, fk, fo, F in classes(args.n, P, f):
                B = L.kenum_bits(proto, args.n, args.m, F)
                tag = dict(f=f, commander_faulty=f0, faulty_king_lieutenants=fk, other_faulty_lieutenants=fo)
                if B > cap:
                    print(json.dumps({"proto": args.proto, "n": args.n, "m": args.m, "faulty_mask": F,
                                      "bits": B, "skipped": f"more than {cap} bits", **tag}), flush=True)
                    continue
                for o in args.orders:
                    row = run_case(eng, L, torch, proto, args.n, args.m, F, o, args)
                    row.update(tag)
                    print(json.dumps(row), flush=True)
    finally:
        eng.close()


def time_kenum(args):
    import torch
    from ba_amd import lib as L
    n, m, F, o, S, T = 7, 1, 0b0001000, 1, 1 << 30, 1 << 20
    assert L.kenum_bits(1, n, m, F) == 36
    eng = L.Engine(args.device)
    try:
        s = torch.cuda.current_stream().cuda_stream
        fm = torch.full((T,), F, dtype=torch.int32, device="cuda")
        oc = torch.full((T,), o, dtype=torch.uint8, device="cuda")
        cnt = torch.zeros(16, dtype=torch.int64, device="cuda")
        wit = torch.full((1,), -1, dtype=torch.int64, device="cuda")
        p = L.make_params(n, m)

        def kenum():
            eng.run_kenum_device(p, 1, F, o, S, d_counters=cnt.data_ptr(), d_witness=wit.data_ptr(), stream=s)

        def king3():
            eng.run_king3_device(p, T, L.KING_SPLIT, d_faulty=fm.data_ptr(), d_order=oc.data_ptr(),
                                 d_counters=cnt.data_ptr(), stream=s)

        kernels = (("k_kenum", kenum, S), ("k_king3", king3, T))
        ms = time_alternating(eng, torch, [(name, name, fn) for name, fn, _ in kernels], args.repeats)
        per = {}
        for name, _, count in kernels:
            med = statistics.median(ms[name])
            per[name] = med * 1e-3 / count
            print(json.dumps({"kernel": name + (" split, staged GIVEN inputs" if name == "k_king3" else " KING3"),
                              "n": n, "m": m, "faulty_mask": F, "order": o, "trials": count,
                              "outputs": "off", "runs_ms": [round(x, 4) for x in ms[name]],
                              "median_ms": round(med, 4),
                              "trials_per_s": float(f"{count / (med * 1e-3):.4e}")}), flush=True)
        print(json.dumps({"ratio": "k_kenum seconds per strategy / k_king3 seconds per trial",
                          "value": float(f"{per['k_kenum'] / per['k_king3']:.4e}")}), flush=True)
    finally:
        eng.close()


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--proto", choices=sorted(PROTOS), default="king")
    ap.add_argument("--n", type=int, default=5)
    ap.add_argument("--m", type=int, default=1)
    ap.add_argument("--f", type=int, nargs="+", default=[1])
    ap.add_argument("--orders", type=int, nargs="+", default=[0, 1])
    ap.add_argument("--chunk", type=lambda v: int(v, 0), default=1 << 34,
                    help="strategies per device call (a multiple of 64)")
    ap.add_argument("--call-limit", type=float, default=30.0, help="seconds one call may take")
    ap.add_argument("--case-budget", type=float, default=120.0, help="seconds one case may take")
    ap.add_argument("--max-bits", type=int, default=44)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--time", action="store_true", help="time k_kenum against k_king3 instead of sweeping")
    ap.add_argument("--repeats", type=int, default=7)
    args = ap.parse_args()
    (time_kenum if args.time else sweep)(args)


if __name__ == "__main__":
    main()
