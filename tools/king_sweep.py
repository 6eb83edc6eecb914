#!/usr/bin/env python3
"""Phase King beside OM(m) and SM(m) over the fault fraction, and the kernel's rate.

Sweep (default): for one (n, m) run f = 0..n traitors (FAULTY_EXACT, random orders)
through Engine.run (OM(m), where its tree is admitted), Engine.run_sm and
Engine.run_king under both policies on the same seed -- all see the same faulty sets
and orders (docs/SEMANTICS.md §9) -- and print one JSON line per f with each
protocol's agreement, validity, in-bound and bound-violation rates, and for Phase
King the share of trials the loyal generals never settle in.

    python tools/king_sweep.py --n 9 --m 2 --trials 65536

--time: k_king on staged inputs (f ~ U{0..m} traitors), 1,048,576 trials per launch,
through Engine.run_king_device, COIN and SPLIT at every --time-shape, with k_sm and
the OM coin engine at the first shape as reference points; HIP events over a window
of at least --window seconds after a warm-up of the same length.  Beside each k_king
rate: the Philox calls per word the kernel issues on these very inputs (counted here
from the staged faulty sets: a wave issues a group of calls for all 64 lanes when any
lane's sender is faulty in the word), ba_king_coin_calls, and for COIN the time the
bare Philox stream (tools/philox_bench, run first as a child process; or
--philox-rate) needs for the issued calls.
"""
from __future__ import annotations

import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "byzantine-agreement_amd"))


def rates(c):
    t, appl = c["trials"], c["validity_applicable"]
    return {"agreement": c["agreement"] / t, "validity": c["validity"] / appl if appl else None,
            "in_bound": c["in_bound"] / t, "bound_violations": c["bound_violations"] / t}


def sweep(args):
    import numpy as np
    from ba_amd import lib as L
    eng = L.Engine(args.device)
    try:
        for f in range(args.n + 1):
            kw = dict(seed=args.seed, faulty_mode=L.FAULTY_EXACT, f=f, order_mode=L.ORDER_RANDOM,
                      want_decisions=False, want_outcome=False)
            row = {"n": args.n, "m": args.m, "f": f, "trials": args.trials}
            try:
                row["om"] = rates(eng.run(args.n, args.m, args.trials, **kw).counters)
            except L.BAError as e:  # the relay tree is too large for this (n, m)
                row["om"] = None
                row["om_error"] = e.code
            row["sm"] = rates(eng.run_sm(args.n, args.m, args.trials, **kw).counters)
            for name, pol in (("king_coin", L.KING_COIN), ("king_split", L.KING_SPLIT)):
                r = eng.run_king(args.n, args.m, args.trials, pol, want_settled=True, **kw)
                row[name] = rates(r.counters)
                row[name]["unsettled"] = float(np.mean(r.settled == L.KING_UNSETTLED))
                done = r.settled[r.settled != L.KING_UNSETTLED]
                row[name]["mean_settled_phase"] = float(done.mean()) if len(done) else None
            print(json.dumps(row), flush=True)
    finally:
        eng.close()


def philox_rates(args):
    """{waves/SIMD: best calls/s} of the bare Philox stream (tools/philox_bench, a child process)."""
    if args.philox_rate:
        return {}, args.philox_rate
    exe = os.path.join(ROOT, "tools", "philox_bench")
    if not os.path.exists(exe):
        sys.exit("tools/philox_bench not built (hipcc -O3 --offload-arch=gfx950 tools/philox_bench.hip "
                 "-o tools/philox_bench) and no --philox-rate given")
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300, check=True).stdout
    best = {}
    for line in out.splitlines():
        if line.startswith("{"):
            r = json.loads(line)
            print(json.dumps({"philox_bench": r}), flush=True)
            w = r["waves_per_simd"]
            if w not in best or r["philox_calls_per_s"] > best[w]:
                best[w] = r["philox_calls_per_s"]
    return best, 0.0


def issued_calls(n, m, fm):
    """Mean Philox calls per 64-trial word k_king issues on the staged faulty masks fm
    (numpy uint32): (lane calls = 64 per issued wave call, wave calls)."""
    import numpy as np
    from ba_amd import lib as L
    P, npairs = L.king_phases(n, m), (n + 1) // 2
    words = fm[:len(fm) // 64 * 64].reshape(-1, 64)
    anyF = np.bitwise_or.reduce(words, axis=1)  # bit j: sender j faulty somewhere in the word
    F = ((anyF[:, None] >> np.arange(32)[None, :]) & 1).astype(bool)
    wave = F[:, 0].astype(np.int64)  # the commander's send
    for v0 in range(0, npairs, 8):
        G = min(4, (npairs - v0 + 1) // 2)
        us = [u for g in range(G) for u in (v0 + 2 * g, v0 + 2 * g + 1) if u < npairs]
        js = [j for u in us for j in (2 * u, 2 * u + 1) if j < n]
        wave += P * G * F[:, js].any(axis=1)  # a group is drawn when any of its senders is faulty
    wave += F[:, :P].sum(axis=1)  # king rounds
    return float(wave.mean() * 64), float(wave.mean())


def timed(args, torch, launch):
    def window(k):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(k):
            launch()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) * 1e-3

    window(20)
    per = window(50) / 50
    k = max(50, int(args.window / per) + 1)
    while True:
        warm = window(k)  # warm-up: the clock settles under this load
        rows = [window(k) for _ in range(args.repeats)]
        sec = min(rows)
        if sec >= args.window:
            return k, sec, rows
        k = int(k * args.window / min(sec, warm) * 1.05) + 1


def time_king(args):
    by_occ, fixed = philox_rates(args)  # before this process opens the GPU itself
    import torch
    from ba_amd import lib as L
    T = args.time_trials
    eng = L.Engine(args.device)
    try:
        s = torch.cuda.current_stream().cuda_stream
        dec = torch.empty(T, dtype=torch.int64, device="cuda")
        out = torch.empty(T, dtype=torch.uint8, device="cuda")
        cnt = torch.zeros(16, dtype=torch.int64, device="cuda")
        for idx, (n, m) in enumerate(args.time_shape):
            kw = dict(seed=args.seed, faulty_mode=L.FAULTY_RANDOM, f=m, order_mode=L.ORDER_RANDOM)
            fm = torch.empty(T, dtype=torch.int32, device="cuda")
            oc = torch.empty(T, dtype=torch.uint8, device="cuda")
            eng.gen_inputs_device(L.make_params(n, m, **kw), T, d_faulty=fm.data_ptr(),
                                  d_order=oc.data_ptr(), stream=s)
            torch.cuda.synchronize()
            p = L.make_params(n, m, seed=args.seed)
            io = dict(d_faulty=fm.data_ptr(), d_order=oc.data_ptr(), d_decisions=dec.data_ptr(),
                      d_outcome=out.data_ptr(), d_counters=cnt.data_ptr(), stream=s)
            lane_calls, wave_calls = issued_calls(n, m, fm.cpu().numpy().view("uint32"))
            # the Philox reference is taken at 4 waves/SIMD, the next occupancy
            # philox_bench measures above the 3 the coin kernel's registers allow
            runs = [("k_king/COIN", lambda: eng.run_king_device(p, T, L.KING_COIN, **io), 4),
                    ("k_king/SPLIT", lambda: eng.run_king_device(p, T, L.KING_SPLIT, **io), 4)]
            if idx == 0:
                runs += [("k_sm", lambda: eng.run_sm_device(p, T, **io), 4),
                         ("om_coin_engine", lambda: eng.run_device(p, T, **io), 0)]
            for name, launch, occ in runs:
                k, sec, rows = timed(args, torch, launch)
                row = {"kernel": name, "n": n, "m": m, "f_max": m, "trials_per_launch": T, "launches": k,
                       "window_s": round(sec, 4), "windows_s": [round(r, 4) for r in rows],
                       "us_per_launch": round(sec / k * 1e6, 2),
                       "trials_per_s": float(f"{k * T / sec:.4e}")}
                if name.startswith("k_king"):
                    row["phases"] = L.king_phases(n, m)
                    row["king_coin_calls_per_word"] = L.king_coin_calls(n, m)
                if name == "k_king/COIN":
                    rate = fixed or by_occ.get(occ) or max(by_occ.values())
                    bound_s = lane_calls * ((T + 63) // 64) / rate
                    row.update({"issued_wave_calls_per_word": round(wave_calls, 2),
                                "issued_lane_calls_per_word": round(lane_calls, 1),
                                "philox_calls_per_s": rate, "philox_waves_per_simd": occ,
                                "bound_philox_us_per_launch": round(bound_s * 1e6, 2),
                                "share_of_philox_bound": round(bound_s / (sec / k), 4)})
                print(json.dumps(row), flush=True)
        torch.cuda.synchronize()
    finally:
        eng.close()


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--n", type=int, default=9)
    ap.add_argument("--m", type=int, default=2)
    ap.add_argument("--trials", type=int, default=65536)
    ap.add_argument("--seed", type=int, default=0xBA5EED)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--time", action="store_true", help="time k_king instead of sweeping")
    ap.add_argument("--time-shape", type=lambda v: tuple(int(x, 0) for x in v.split(",")), nargs="+",
                    default=[(10, 3), (32, 7)], metavar="N,M")
    ap.add_argument("--time-trials", type=int, default=1 << 20)
    ap.add_argument("--window", type=float, default=0.5, help="seconds per timed window")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--philox-rate", type=float, default=0.0, help="Philox calls/s (skip philox_bench)")
    args = ap.parse_args()
    (time_king if args.time else sweep)(args)


if __name__ == "__main__":
    main()
