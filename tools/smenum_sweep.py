#!/usr/bin/env python3
"""Exhaustive enumeration of a traitor coalition's strategies against SM(m)
(docs/SEMANTICS.md §12), and the k_smenum kernel's rate.

Sweep (default): for (n, m) and each f in --f, one representative faulty set per class
with f traitors, for the orders retreat and attack and for both forms (messages,
coalition).  A class is (commander faulty or not, number of faulty lieutenants);
relabelling the lieutenants is a symmetry of the protocol, and the representative
takes the lowest indices.  Cases above --max-bits (and above the library's 48) are
listed as skipped.  The whole space 2^B is walked through Engine.run_smenum_device in
calls of --chunk strategies; every call is synchronised and timed on its own, and a
call that took longer than --call-limit seconds, or a case that has used --case-budget
seconds, ends the case there: its line then says how far it got ("complete": false).
One JSON line per case: B, strategies, the counters, the witness, seconds and
strategies per second.  The lines go to standard output and are appended to --out
(default profiles/smenum_sweep_n<n>_m<m>.jsonl).

These limits are checked when a call has returned: they cannot end a launch that never
returns.  That bound has to come from outside the process: run the tool under
`timeout -k`, sized to the cases asked for.

    timeout -k 10 300 python tools/smenum_sweep.py --n 7 --m 3 --f 1 2 3

--masks 0x7 0xF: these faulty sets instead of the classes of --f.

--time: one launch of 2^30 strategies, counters only, of k_smenum in the coalition form
at (10, 3), F = {0,1,2} (42 bits) and in the message form at (7, 3), F = {0,1,2} (40
bits), next to k_kenum Phase King at (9, 2), F = {7,8} (42 bits).  The three alternate
run by run; each run is timed by the library's own HIP events (ba_profile_enable); the
lines give every run, the median and strategies per second.
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

FORMS = {"messages": 0, "coalition": 1}


def classes(n, f):
    """[(F_0, faulty lieutenants, mask)] with f traitors in all."""
    out = []
    for f0 in (0, 1):
        fl = f - f0
        if 0 <= fl <= n - 1:
            out.append((f0, fl, f0 | (((1 << fl) - 1) << 1)))
    return out


def emit(args, row):
    line = json.dumps(row)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as fh:
            fh.write(line + "\n")


def run_case(eng, L, torch, form, n, m, F, o, args):
    def call(first, count, d_cnt, d_wit, stream):
        eng.run_smenum_device(L.make_params(n, m, first_trial=first), form, F, o, count, d_counters=d_cnt,
                              d_witness=d_wit, stream=stream)

    def messages(w):
        return {"witness_messages": None if w is None else L.decode_smstrategy(form, n, m, F, o, w)}

    head = {"form": [k for k, v in FORMS.items() if v == form][0], "n": n, "m": m, "faulty_mask": F, "order": o}
    return walk(call, L, torch, head, L.smenum_bits(form, n, m, F), args, messages)


def sweep(args):
    import torch
    from ba_amd import lib as L
    eng = L.Engine(args.device)
    try:
        eng.run_smenum(0, 4, 1, 0b0011, 1)  # warm-up: module load
        cap = min(args.max_bits, L.ENUM_MAX_BITS)
        if args.masks:
            cases = [(F & 1, bin(F >> 1).count("1"), F) for F in args.masks]
        else:
            cases = [c for f in args.f for c in classes(args.n, f)]
        for f0, fl, F in cases:
            tag = dict(f=f0 + fl, commander_faulty=f0, faulty_lieutenants=fl)
            for name in args.forms:
                form = FORMS[name]
                B = L.smenum_bits(form, args.n, args.m, F)
                if B > cap:
                    emit(args, {"form": name, "n": args.n, "m": args.m, "faulty_mask": F, "bits": B,
                                "skipped": f"more than {cap} bits", **tag})
                    continue
                for o in args.orders:
                    row = run_case(eng, L, torch, form, args.n, args.m, F, o, args)
                    row.update(tag)
                    emit(args, row)
    finally:
        eng.close()


def time_smenum(args):
    import torch
    from ba_amd import lib as L
    S, o = 1 << 30, 1
    sm_c = (L.SMENUM_COALITION, 10, 3, 0b0000000111)
    sm_m = (L.SMENUM_MESSAGES, 7, 3, 0b0000111)
    kk = (L.KENUM_KING, 9, 2, 0b110000000)
    assert L.smenum_bits(*sm_c) == 42 and L.smenum_bits(*sm_m) == 40 and L.kenum_bits(*kk) == 42
    eng = L.Engine(args.device)
    try:
        s = torch.cuda.current_stream().cuda_stream
        cnt = torch.zeros(16, dtype=torch.int64, device="cuda")
        wit = torch.full((1,), -1, dtype=torch.int64, device="cuda")

        def smenum(case):
            form, n, m, F = case
            return lambda: eng.run_smenum_device(L.make_params(n, m), form, F, o, S, d_counters=cnt.data_ptr(),
                                                 d_witness=wit.data_ptr(), stream=s)

        def kenum():
            proto, n, m, F = kk
            eng.run_kenum_device(L.make_params(n, m), proto, F, o, S, d_counters=cnt.data_ptr(),
                                 d_witness=wit.data_ptr(), stream=s)

        kernels = (("k_smenum coalition", "k_smenum", smenum(sm_c), sm_c),
                   ("k_smenum messages", "k_smenum", smenum(sm_m), sm_m), ("k_kenum KING", "k_kenum", kenum, kk))
        ms = time_alternating(eng, torch, [(what, name, fn) for what, name, fn, _ in kernels], args.repeats)
        for what, _, _, (_, n, m, F) in kernels:
            med = statistics.median(ms[what])
            emit(args, {"kernel": what, "n": n, "m": m, "faulty_mask": F, "order": o, "strategies": S,
                        "outputs": "off", "runs_ms": [round(x, 4) for x in ms[what]],
                        "median_us_per_launch": round(med * 1e3, 1),
                        "strategies_per_s": float(f"{S / (med * 1e-3):.4e}")})
    finally:
        eng.close()


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--n", type=int, default=5)
    ap.add_argument("--m", type=int, default=2)
    ap.add_argument("--f", type=int, nargs="+", default=[1, 2])
    ap.add_argument("--masks", type=lambda v: int(v, 0), nargs="+", default=None,
                    help="faulty sets to run instead of the classes of --f")
    ap.add_argument("--forms", choices=sorted(FORMS), nargs="+", default=["messages", "coalition"])
    ap.add_argument("--orders", type=int, nargs="+", default=[0, 1])
    ap.add_argument("--chunk", type=lambda v: int(v, 0), default=1 << 36,
                    help="strategies per device call (a multiple of 64)")
    ap.add_argument("--call-limit", type=float, default=30.0, help="seconds one call may take")
    ap.add_argument("--case-budget", type=float, default=120.0, help="seconds one case may take")
    ap.add_argument("--max-bits", type=int, default=44)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--out", default=None, help="jsonl file the lines are appended to; '' for none")
    ap.add_argument("--time", action="store_true", help="time k_smenum next to k_kenum instead of sweeping")
    ap.add_argument("--repeats", type=int, default=7)
    args = ap.parse_args()
    if args.out is None:
        args.out = os.path.join(ROOT, "profiles", "smenum_time.jsonl" if args.time
                                else f"smenum_sweep_n{args.n}_m{args.m}.jsonl")
    (time_smenum if args.time else sweep)(args)


if __name__ == "__main__":
    main()
