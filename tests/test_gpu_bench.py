"""GPU test of a plain bench.py run: the headline line only, --steps timed steps, and
--dump-outputs files that hold the last timed step's results (checked on the oracle)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import oracle_c

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.gpu
def test_plain_run_dumps_the_last_timed_step(tmp_path):
    """bench.py --steps 3 --dump-outputs DIR at a small batch: the line carries the
    headline fields and none of --full's; the counters are those of exactly 3 steps;
    the dumped decisions, outcomes and trial indices are the third timed step's, bit
    for bit what the oracle computes for those trials."""
    steps, warmup, B, seed = 3, 1, 64 * 40, 0xBA5EED
    d = tmp_path / "out"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps",
                        str(steps), "--warmup", str(warmup), "--batch", str(B), "--warm-s", "0",
                        "--dump-outputs", str(d)],
                       capture_output=True, text=True, timeout=120, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    (line,) = [json.loads(x) for x in r.stdout.splitlines() if x.startswith("{")]
    assert line["steps"] == steps and line["ms_per_step"] > 0 and line["value"] > 0
    assert line["unit"] == "trial-decisions/s" and line["higher_is_better"] is True
    assert line["dtype"] == "u64" and line["full"] is False
    for k in ("cpu_baseline", "roofline", "value_single_stream", "clock", "kernels_ms"):
        assert k not in line
    assert line["counters"]["trials"] == steps * B
    assert sorted(line["outputs_dumped"]["files"]) == sorted(os.listdir(d))
    got = {f[:-4]: np.load(d / f) for f in os.listdir(d)}
    assert all(a.dtype in (np.float32, np.float64) for a in got.values())
    # the timed steps follow the warmup + 2 warm-up slots; the last one is slot warmup + 2 + steps - 1
    first = (warmup + 2 + steps - 1) * B
    assert np.array_equal(got["trial_index"], first + np.arange(B))
    kw = dict(seed=seed, faulty_mode=1, f=3, order_mode=1)
    od, oo, _ = oracle_c.run(10, 3, B, first_trial=first, **kw)
    words = (got["decisions_hi"].astype(np.uint64) << np.uint64(32)) | got["decisions_lo"].astype(np.uint64)
    assert np.array_equal(words, od) and np.array_equal(got["outcome"], oo)
    _, _, oc = oracle_c.run(10, 3, steps * B, first_trial=(warmup + 2) * B, **kw)
    assert {k: line["counters"][k] for k in oc} == oc
    assert {k: int(got["counters"][i]) for i, k in enumerate(oracle_c.COUNTER_NAMES)} == oc
