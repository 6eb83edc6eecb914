"""What enum_sweep.py, kenum_sweep.py, smenum_sweep.py and renum_sweep.py share: the
chunked walk of one case's strategy space through a device entry, and the alternating
timed loop of --time."""
from __future__ import annotations

import time


def run_case(call, L, torch, head, bits, args, witness_extra=None, stats=None):
    """Walk the 2^bits strategies of one case in calls of args.chunk strategies.
    call(first, count, d_counters, d_witness, stream) queues one device call; every call is
    synchronised and timed on its own, and a call that took longer than args.call_limit
    seconds, or a case that has used args.case_budget seconds, ends the case there.
    Returns the case's JSON row: `head` (the keys that name the case), then bits,
    strategies, covered, complete, counters, witness, what witness_extra(witness) adds,
    calls, seconds, slowest_call_s and strategies_per_s.
    stats = (words, indices preset to all-ones, to_row): the case also accumulates a
    tensor of `words` uint64 on the device, which call() takes as a sixth argument, and
    the row gains what to_row(list of the words) returns (renum_sweep.py's stats)."""
    total = 1 << bits
    cnt = torch.zeros(16, dtype=torch.int64, device="cuda")
    wit = torch.full((1,), -1, dtype=torch.int64, device="cuda")
    s = torch.cuda.current_stream().cuda_stream
    more = ()
    if stats:
        sts = torch.zeros(stats[0], dtype=torch.int64, device="cuda")
        for i in stats[1]:
            sts[i] = -1
        more = (sts.data_ptr(),)
    done, secs, calls, slowest = 0, 0.0, 0, 0.0
    while done < total:
        nt = min(args.chunk, total - done)
        t0 = time.perf_counter()
        call(done, nt, cnt.data_ptr(), wit.data_ptr(), s, *more)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        done += nt
        secs += dt
        calls += 1
        slowest = max(slowest, dt)
        if dt > args.call_limit or secs > args.case_budget:
            break
    c = dict(zip(L.COUNTER_NAMES, cnt.cpu().tolist()))
    w = int(wit.cpu().numpy().view("uint64")[0])
    w = None if w == L.NO_WITNESS else w
    return {**head, "bits": bits, "strategies": total, "covered": done, "complete": done == total,
            "counters": c, "witness": w, **(witness_extra(w) if witness_extra else {}),
            **(stats[2](sts.cpu().numpy().view("uint64").tolist()) if stats else {}), "calls": calls,
            "seconds": round(secs, 4), "slowest_call_s": round(slowest, 4),
            "strategies_per_s": float(f"{done / secs:.4e}") if secs > 0 else None}


def time_alternating(eng, torch, kernels, repeats):
    """kernels: [(key, profile name, fn)], fn() queues one launch.  After one warm-up run
    of each, the kernels alternate run by run; each run is timed by the library's own HIP
    events (ba_profile_enable).  Returns {key: [milliseconds of every run]}."""
    for _, _, fn in kernels:  # warm-up
        fn()
    torch.cuda.synchronize()
    ms = {key: [] for key, _, _ in kernels}
    for _ in range(repeats):
        for key, name, fn in kernels:
            eng.profile(True)
            fn()
            torch.cuda.synchronize()
            launches, total = eng.profile_read()[name]
            assert launches == 1
            ms[key].append(total)
    eng.profile(False)
    return ms
