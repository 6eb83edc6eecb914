#!/usr/bin/env python3
"""SM(m) against OM(m) over the fault fraction, and the SM kernel's rate.

Sweep (default): for one (n, m) run f = 0..n traitors (FAULTY_EXACT, random orders)
through Engine.run (oral messages) and Engine.run_sm (signed messages) on the same
seed -- the two see the same faulty sets and orders (docs/SEMANTICS.md §6) -- and
print one JSON line per f with each protocol's agreement, validity and
bound-violation rates.

    python tools/sm_sweep.py --n 4 --m 2 --trials 65536

--time: k_sm at n = 10, m = 3, 1,048,576 trials per launch (--time-shape: another shape) through
Engine.run_sm_device on staged inputs, with and without V sets, timed with HIP
events over a window of at least --window seconds after a warm-up of the same
length.  Each rate is printed beside two computed bounds:
  philox : ba_sm_coin_calls x words over the bare Philox stream rate that
           tools/philox_bench (run first, as a child process; or --philox-rate)
           measured in this same run;
  hbm    : 14 B per trial (5 B of staged inputs read, 9 B of decisions and outcome
           written), 22 B with V sets, over the HBM peak (--hbm-peak, 8 TB/s);
and the line says which of the two binds (the lower one) and the share reached.
"""
from __future__ import annotations

import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "byzantine-agreement_amd"))


def sweep(args):
    from ba_amd import lib as L
    eng = L.Engine(args.device)
    try:
        for f in range(args.n + 1):
            kw = dict(seed=args.seed, faulty_mode=L.FAULTY_EXACT, f=f, order_mode=L.ORDER_RANDOM,
                      want_decisions=False, want_outcome=False)
            row = {"n": args.n, "m": args.m, "f": f, "trials": args.trials}
            for name, run in (("om", eng.run), ("sm", eng.run_sm)):
                c = run(args.n, args.m, args.trials, **kw).counters
                t, appl = c["trials"], c["validity_applicable"]
                row[name] = {
                    "agreement": c["agreement"] / t,
                    "validity": c["validity"] / appl if appl else None,
                    "in_bound": c["in_bound"] / t,
                    "bound_violations": c["bound_violations"] / t,
                    "undefined_decisions_per_trial": c["undefined_decisions"] / t,
                }
            print(json.dumps(row), flush=True)
    finally:
        eng.close()


def philox_rate(args):
    """(calls/s, source) of the bare Philox stream: the best code shape at the
    occupancy k_sm runs at (tools/philox_bench, a child process)."""
    if args.philox_rate:
        return args.philox_rate, "--philox-rate"
    exe = os.path.join(ROOT, "tools", "philox_bench")
    if not os.path.exists(exe):
        sys.exit("tools/philox_bench not built (hipcc -O3 --offload-arch=gfx950 tools/philox_bench.hip "
                 "-o tools/philox_bench) and no --philox-rate given")
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300, check=True).stdout
    best = None
    for line in out.splitlines():
        if line.startswith("{"):
            r = json.loads(line)
            print(json.dumps({"philox_bench": r}), flush=True)
            if r["waves_per_simd"] == args.waves_per_simd and (
                    best is None or r["philox_calls_per_s"] > best["philox_calls_per_s"]):
                best = r
    return best["philox_calls_per_s"], f"philox_bench {best['variant']} at {best['waves_per_simd']} waves/SIMD"


def time_sm(args):
    rate, src = philox_rate(args)  # before this process opens the GPU itself
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
        vs = torch.empty(T, dtype=torch.int64, device="cuda")
        cnt = torch.zeros(16, dtype=torch.int64, device="cuda")
        eng.gen_inputs_device(L.make_params(n, m, **kw), T, d_faulty=fm.data_ptr(), d_order=oc.data_ptr(),
                              stream=s)
        p = L.make_params(n, m, seed=args.seed)
        calls = L.sm_coin_calls(n, m) * ((T + 63) // 64)

        def launches(k, vsets):
            for _ in range(k):
                eng.run_sm_device(p, T, d_faulty=fm.data_ptr(), d_order=oc.data_ptr(),
                                  d_decisions=dec.data_ptr(), d_outcome=out.data_ptr(),
                                  d_vsets=vs.data_ptr() if vsets else 0, d_counters=cnt.data_ptr(),
                                  stream=s)

        def window(k, vsets):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            launches(k, vsets)
            e1.record()
            e1.synchronize()
            return e0.elapsed_time(e1) * 1e-3

        for vsets in (False, True):
            launches(20, vsets)
            torch.cuda.synchronize()
            per = window(50, vsets) / 50
            k = max(50, int(args.window / per) + 1)
            while True:
                warm = window(k, vsets)  # warm-up: the clock settles under this load
                rows = [window(k, vsets) for _ in range(args.repeats)]
                sec = min(rows)
                if sec >= args.window:
                    break
                k = int(k * args.window / min(sec, warm) * 1.05) + 1  # launches sped up: a longer run
            tps = k * T / sec
            bytes_per_trial = 22 if vsets else 14
            b_philox = T / (calls / rate)
            b_hbm = args.hbm_peak / bytes_per_trial
            binding = "philox" if b_philox < b_hbm else "hbm"
            print(json.dumps({
                "kernel": "k_sm", "n": n, "m": m, "f_max": f, "trials_per_launch": T, "vsets": vsets,
                "launches": k, "window_s": round(sec, 4), "windows_s": [round(r, 4) for r in rows],
                "us_per_launch": round(sec / k * 1e6, 2), "trials_per_s": float(f"{tps:.4e}"),
                "coin_calls_per_word": L.sm_coin_calls(n, m),
                "bound_philox_trials_per_s": float(f"{b_philox:.4e}"),
                "philox_calls_per_s": rate, "philox_source": src,
                "bound_hbm_trials_per_s": float(f"{b_hbm:.4e}"), "bytes_per_trial": bytes_per_trial,
                "hbm_peak_bytes_per_s": args.hbm_peak, "binding_bound": binding,
                "share_of_binding_bound": round(tps / min(b_philox, b_hbm), 4),
            }), flush=True)
        torch.cuda.synchronize()
    finally:
        eng.close()


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--n", type=int, default=4)
    ap.add_argument("--m", type=int, default=2)
    ap.add_argument("--trials", type=int, default=65536)
    ap.add_argument("--seed", type=int, default=0xBA5EED)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--time", action="store_true", help="time k_sm instead of sweeping")
    ap.add_argument("--time-shape", type=lambda v: tuple(int(x, 0) for x in v.split(",")),
                    default=(10, 3, 3, 1 << 20), metavar="N,M,F,TRIALS",
                    help="--time: another shape (f ~ U{0..F} traitors), e.g. 32,8,8,1048576")
    ap.add_argument("--window", type=float, default=0.5, help="seconds per timed window")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--philox-rate", type=float, default=0.0, help="Philox calls/s (skip philox_bench)")
    ap.add_argument("--waves-per-simd", type=int, default=4, help="k_sm's occupancy (128 VGPRs)")
    ap.add_argument("--hbm-peak", type=float, default=8e12)
    args = ap.parse_args()
    (time_sm if args.time else sweep)(args)


if __name__ == "__main__":
    main()
