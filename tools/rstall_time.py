#!/usr/bin/env python3
"""k_rstall's time per launch beside k_rand under BA_KING_SPLIT (docs/SEMANTICS.md §15, §13).

1,048,576 trials per launch on staged inputs, at every --shape and every --phases R, both
coins.  Two staged input sets, as tools/rand_sweep.py --time has them: "exact" has f = m
traitors in every trial, so every word is in bound and the early finish can fire; "mixed"
is FAULTY_RANDOM with f = n, which puts an out-of-bound trial into every word (the share
of such words is printed), so every word runs all its phases.  At each point k_rstall and
k_rand SPLIT alternate launch by launch in one run (enum_common.time_alternating), each
timed by the library's own HIP events; median, minimum and maximum over --repeats runs.
k_rand takes up to 64 phases: beyond, k_rstall is timed alone.

Beside each k_rstall time: ba_rstall_coin_calls, the distinct Philox calls per word when
every toss is drawn, and the time the bare Philox stream needs for them at --philox-rate
lane calls/s; and the same for the calls a wave issues (one call per phase, for all 64
lanes, whichever the coin).
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


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--shape", type=lambda v: tuple(int(x, 0) for x in v.split(",")), nargs="+",
                    default=[(10, 3), (32, 10)], metavar="N,M")
    ap.add_argument("--phases", type=int, nargs="+", default=[16, 250])
    ap.add_argument("--trials", type=int, default=1 << 20)
    ap.add_argument("--repeats", type=int, default=15)
    ap.add_argument("--seed", type=int, default=0xBA5EED)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--philox-rate", type=float, default=1.055e12,
                    help="bare Philox stream, lane calls/s (profiles/r18a_rand_time.jsonl, DESIGN.md §21)")
    args = ap.parse_args()
    import numpy as np
    import torch
    from ba_amd import lib as L
    T = args.trials
    words = (T + 63) // 64
    eng = L.Engine(args.device)
    try:
        s = torch.cuda.current_stream().cuda_stream
        dec = torch.empty(T, dtype=torch.int64, device="cuda")
        out = torch.empty(T, dtype=torch.uint8, device="cuda")
        cnt = torch.zeros(16, dtype=torch.int64, device="cuda")
        for n, m in args.shape:
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

            for R in args.phases:
                kernels, meta = [], {}
                for cname, coin in (("LOCAL", L.RAND_LOCAL), ("COMMON", L.RAND_COMMON)):
                    for inp in ("exact", "mixed"):
                        key = f"k_rstall/{cname}/{inp}"
                        kernels.append((key, "k_rstall", lambda coin=coin, inp=inp:
                                        eng.run_rstall_device(p, T, R, coin, **io(inp))))
                        meta[key] = {"inputs": inp, "coin_calls_per_word": L.rstall_coin_calls(n, R, coin)}
                        if R <= L.RAND_MAX_PHASES:
                            key = f"k_rand/SPLIT/{cname}/{inp}"
                            kernels.append((key, "k_rand", lambda coin=coin, inp=inp:
                                            eng.run_rand_device(p, T, R, L.KING_SPLIT, coin, **io(inp))))
                            meta[key] = {"inputs": inp, "coin_calls_per_word": R * (n if coin == L.RAND_LOCAL else 1)}
                ms = time_alternating(eng, torch, kernels, args.repeats)
                for key, _, _ in kernels:
                    v = sorted(ms[key])
                    med = v[len(v) // 2] * 1e3
                    row = {"kernel": key, "n": n, "m": m, "phases": R, "trials_per_launch": T, "runs": len(v),
                           **meta[key], "words_with_out_of_bound_trial": ins[meta[key]["inputs"]][2],
                           "median_us_per_launch": round(med, 2), "min_us_per_launch": round(v[0] * 1e3, 2),
                           "max_us_per_launch": round(v[-1] * 1e3, 2), "us_per_phase": round(med / R, 3)}
                    if key.startswith("k_rstall"):
                        other = ms.get(key.replace("k_rstall", "k_rand/SPLIT"))
                        if other:
                            o = sorted(other)
                            row["k_rand_split_median_us"] = round(o[len(o) // 2] * 1e3, 2)
                            row["k_rand_split_max_minus_min_us"] = round((o[-1] - o[0]) * 1e3, 2)
                            row["time_over_k_rand_split"] = round(med / (o[len(o) // 2] * 1e3), 4)
                        bound = meta[key]["coin_calls_per_word"] * words / args.philox_rate * 1e6
                        issued = R * 64 * words / args.philox_rate * 1e6
                        row.update({"philox_lane_calls_per_s": args.philox_rate,
                                    "bound_philox_us": round(bound, 3),
                                    "bound_share_of_time": round(bound / med, 4) if med else None,
                                    "issued_wave_calls_per_word_full_run": R,
                                    "issued_philox_us_full_run": round(issued, 2),
                                    "issued_share_of_time_full_run": round(issued / med, 4) if med else None})
                    print(json.dumps(row), flush=True)
    finally:
        eng.close()


if __name__ == "__main__":
    main()
