#!/usr/bin/env python3
"""Phase King and KING3 beside OM(m) and SM(m) over the fault fraction, and the
kernels' rates.

Sweep (default): for one (n, m) run f = 0..n traitors (FAULTY_EXACT, random orders)
through Engine.run (OM(m), where its tree is admitted), Engine.run_sm,
Engine.run_king and Engine.run_king3 (the three-round King algorithm), the last two
under both policies, on the same seed -- all see the same faulty sets and orders
(docs/SEMANTICS.md §9, §10) -- and print one JSON line per f with each protocol's
agreement, validity, in-bound and bound-violation rates, and for the two King
protocols the share of trials the loyal generals never settle in.  A protocol whose
entry rejects the shape (m > 8 everywhere but KING3) is null, with its error code.

    python tools/king_sweep.py --n 9 --m 2 --trials 65536

--time: k_king on staged inputs (f ~ U{0..m} traitors), 1,048,576 trials per launch,
through Engine.run_king_device, COIN and SPLIT at every --time-shape, with k_sm and
the OM coin engine at the first shape as reference points; HIP events over a window
of at least --window seconds after a warm-up of the same length; k_king3 (m <= 10)
is timed beside k_king (m <= 8) at every shape, and --time-faulty exact stages exactly
f = m traitors per trial.  us_per_launch is the fastest window's, median_us_per_launch
and spread_us_per_launch (max - min) are over the --repeats windows.  Beside each
k_king / k_king3 rate: the Philox calls per word the kernel issues on these very
inputs (counted here from the staged faulty sets: a wave issues a group of calls for
all 64 lanes when any lane's sender is faulty in the word), ba_king_coin_calls or
ba_king3_coin_calls, and for COIN the time the bare Philox stream
(tools/philox_bench, run first as a child process; or --philox-rate) needs for the
issued calls.
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
            try:
                row["sm"] = rates(eng.run_sm(args.n, args.m, args.trials, **kw).counters)
            except L.BAError as e:  # m > 8
                row["sm"] = None
                row["sm_error"] = e.code
            for name, run, pol in (("king_coin", eng.run_king, L.KING_COIN),
                                   ("king_split", eng.run_king, L.KING_SPLIT),
                                   ("king3_coin", eng.run_king3, L.KING_COIN),
                                   ("king3_split", eng.run_king3, L.KING_SPLIT)):
                try:
                    r = run(args.n, args.m, args.trials, pol, want_settled=True, **kw)
                except L.BAError as e:  # Phase King: m > 8
                    row[name] = None
                    row[name + "_error"] = e.code
                    continue
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


def issued_calls(n, m, fm, king3=False):
    """Mean Philox calls per 64-trial word k_king (k_king3: two all-to-all rounds per
    phase) issues on the staged faulty masks fm (numpy uint32): (lane calls = 64 per
    issued wave call, wave calls)."""
    import numpy as np
    from ba_amd import lib as L
    P, npairs = (L.king3_phases if king3 else L.king_phases)(n, m), (n + 1) // 2
    rounds = 2 if king3 else 1
    words = fm[:len(fm) // 64 * 64].reshape(-1, 64)
    anyF = np.bitwise_or.reduce(words, axis=1)  # bit j: sender j faulty somewhere in the word
    F = ((anyF[:, None] >> np.arange(32)[None, :]) & 1).astype(bool)
    wave = F[:, 0].astype(np.int64)  # the commander's send
    for v0 in range(0, npairs, 8):
        G = min(4, (npairs - v0 + 1) // 2)
        us = [u for g in range(G) for u in (v0 + 2 * g, v0 + 2 * g + 1) if u < npairs]
        js = [j for u in us for j in (2 * u, 2 * u + 1) if j < n]
        wave += P * rounds * G * F[:, js].any(axis=1)  # a group is drawn when any of its senders is faulty
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
            fmode = L.FAULTY_EXACT if args.time_faulty == "exact" else L.FAULTY_RANDOM
            kw = dict(seed=args.seed, faulty_mode=fmode, f=m, order_mode=L.ORDER_RANDOM)
            fm = torch.empty(T, dtype=torch.int32, device="cuda")
            oc = torch.empty(T, dtype=torch.uint8, device="cuda")
            # the inputs do not depend on m (docs/SEMANTICS.md §4), and ba_gen_inputs_device
            # admits m <= 8 only: k_king3's m = 9, 10 are staged under m = 8
            eng.gen_inputs_device(L.make_params(n, min(m, 8), **kw), T, d_faulty=fm.data_ptr(),
                                  d_order=oc.data_ptr(), stream=s)
            torch.cuda.synchronize()
            p = L.make_params(n, m, seed=args.seed)
            io = dict(d_faulty=fm.data_ptr(), d_order=oc.data_ptr(), d_decisions=dec.data_ptr(),
                      d_outcome=out.data_ptr(), d_counters=cnt.data_ptr(), stream=s)
            masks = fm.cpu().numpy().view("uint32")
            # the Philox reference is taken at 4 waves/SIMD, the next occupancy
            # philox_bench measures above the 3 the coin kernels' registers allow
            runs = []
            if m <= 8:
                runs += [("k_king/COIN", lambda: eng.run_king_device(p, T, L.KING_COIN, **io), 4),
                         ("k_king/SPLIT", lambda: eng.run_king_device(p, T, L.KING_SPLIT, **io), 4)]
            runs += [("k_king3/COIN", lambda: eng.run_king3_device(p, T, L.KING_COIN, **io), 4),
                     ("k_king3/SPLIT", lambda: eng.run_king3_device(p, T, L.KING_SPLIT, **io), 4)]
            if idx == 0 and m <= 8:
                runs += [("k_sm", lambda: eng.run_sm_device(p, T, **io), 4),
                         ("om_coin_engine", lambda: eng.run_device(p, T, **io), 0)]
            for name, launch, occ in runs:
                k, sec, rows = timed(args, torch, launch)
                row = {"kernel": name, "n": n, "m": m, "f_max": m, "faulty": args.time_faulty,
                       "trials_per_launch": T, "launches": k,
                       "window_s": round(sec, 4), "windows_s": [round(r, 4) for r in rows],
                       "us_per_launch": round(sec / k * 1e6, 2),
                       "median_us_per_launch": round(sorted(rows)[len(rows) // 2] / k * 1e6, 2),
                       "spread_us_per_launch": round((max(rows) - min(rows)) / k * 1e6, 2),
                       "trials_per_s": float(f"{k * T / sec:.4e}")}
                king3 = name.startswith("k_king3")
                if king3:
                    row["phases"] = L.king3_phases(n, m)
                    row["king3_coin_calls_per_word"] = L.king3_coin_calls(n, m)
                elif name.startswith("k_king"):
                    row["phases"] = L.king_phases(n, m)
                    row["king_coin_calls_per_word"] = L.king_coin_calls(n, m)
                if name.endswith("/COIN"):
                    lane_calls, wave_calls = issued_calls(n, m, masks, king3)
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
    ap.add_argument("--time", action="store_true", help="time k_king and k_king3 instead of sweeping")
    ap.add_argument("--time-faulty", choices=["random", "exact"], default="random",
                    help="staged traitors per trial: f ~ U{0..m} (random) or f = m (exact)")
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
