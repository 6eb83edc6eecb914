"""GPU parity of the trimmed k_om3w bookkeeping against the oracle.

The depth-3 WAVE kernel's Philox groups rotate through register windows, its
pair exchange is one v_cndmask_b32_dpp per dword, and its per-task counter fold
packs two counters per dword and hands the row sums over through LDS
(wave_fold_packed).  None of it may move a bit: decisions, per-trial outcome
bytes and all 12 run counters are compared with oracle_c.run.

Shapes: n in {5, 6, 7, 10, 11, 14} at m = 3 -- both parities of S = n - 3 and
C = n - 2 (both branches of the round's Philox group) and the task widths
W = 64 / C from 21 down to 5.  Batches: 1, 65, one full task, one full task
plus a trial, and five tasks plus 37 trials under BA_WAVE_MAX_BLOCKS=1, where
one wave runs several tasks and the packed fold accumulates across them.  Each
with staged inputs (gen_inputs_device buffers, GIVEN mode) and in-kernel draws.
"""
import numpy as np
import pytest

import oracle_c
from test_gpu import same

pytestmark = pytest.mark.gpu

OM3_N = (5, 6, 7, 10, 11, 14)


def task_words(n):
    return 64 // (n - 2)  # Om3W<N>::W


def run_staged(engine, n, m, B, kw):
    """gen_inputs_device buffers + a GIVEN-mode run on them (the bench's path)."""
    import torch
    from ba_amd import lib as L
    fb = torch.empty(B, dtype=torch.int32, device="cuda")
    ob = torch.empty(B, dtype=torch.uint8, device="cuda")
    dec = torch.empty(B, dtype=torch.int64, device="cuda")
    out = torch.empty(B, dtype=torch.uint8, device="cuda")
    cnt = torch.zeros(16, dtype=torch.int64, device="cuda")
    s = torch.cuda.current_stream().cuda_stream
    engine.gen_inputs_device(L.make_params(n, m, **kw), B, d_faulty=fb.data_ptr(),
                             d_order=ob.data_ptr(), stream=s)
    p = L.make_params(n, m, seed=kw["seed"], first_trial=kw["first_trial"])
    engine.run_device(p, B, d_faulty=fb.data_ptr(), d_order=ob.data_ptr(),
                      d_decisions=dec.data_ptr(), d_outcome=out.data_ptr(),
                      d_counters=cnt.data_ptr(), stream=s)
    torch.cuda.synchronize()
    return dec.cpu().numpy().view(np.uint64), out.cpu().numpy(), cnt.cpu().tolist()[:12]


def check_both(engine, n, m, B, kw, tag):
    from ba_amd import lib as L
    assert L.load().ba_engine_for(n, m) == L.ENGINE_FUSED
    od, oo, ocnt = oracle_c.run(n, m, B, **kw)
    res = engine.run(n, m, B, **kw)
    same(res.decisions, od, "decisions, drawn " + tag)
    same(res.outcome, oo, "outcome, drawn " + tag)
    assert {k: res.counters[k] for k in ocnt} == ocnt, "drawn " + tag
    dec, out, cnt = run_staged(engine, n, m, B, kw)
    same(dec, od, "decisions, staged " + tag)
    same(out, oo, "outcome, staged " + tag)
    assert cnt == list(ocnt.values()), "staged " + tag


@pytest.mark.parametrize("n", OM3_N)
def test_om3w_batches_vs_oracle(monkeypatch, n):
    from ba_amd import lib as L
    W = task_words(n)
    kw = dict(seed=0x7215 + n, faulty_mode=L.FAULTY_RANDOM, f=(n - 1) // 3 + 1,
              order_mode=L.ORDER_RANDOM, first_trial=64 * 9)
    for B, cap in ((1, None), (65, None), (64 * W, None), (64 * W + 1, None),
                   (64 * W * 5 + 37, "1")):
        if cap:
            monkeypatch.setenv("BA_WAVE_MAX_BLOCKS", cap)
        else:
            monkeypatch.delenv("BA_WAVE_MAX_BLOCKS", raising=False)
        e = L.Engine(0)
        try:
            check_both(e, n, 3, B, kw, f"n={n} B={B} cap={cap}")
        finally:
            e.close()


@pytest.mark.parametrize("n", (5, 14))
def test_packed_fold_worst_case_every_general_faulty(monkeypatch, n):
    """Every general faulty: faulty_total is n per trial, the largest sum any
    counter reaches in a task (64 W n, the bound of wave_fold_packed's
    static_assert), and the undefined decisions are as many as the lies make
    them.  Several full tasks, spread over waves and walked by one block."""
    from ba_amd import lib as L
    W = task_words(n)
    B = 64 * W * 3
    fm = np.full(B, (1 << n) - 1, np.uint32)
    oc = np.random.default_rng(n).choice([0, 1, 2], B).astype(np.uint8)
    od, oo, ocnt = oracle_c.run(n, 3, B, seed=11, faulty=fm, order=oc, first_trial=64 * 5)
    assert ocnt["faulty_total"] == n * B
    for cap in (None, "1"):
        if cap:
            monkeypatch.setenv("BA_WAVE_MAX_BLOCKS", cap)
        else:
            monkeypatch.delenv("BA_WAVE_MAX_BLOCKS", raising=False)
        e = L.Engine(0)
        try:
            res = e.run(n, 3, B, seed=11, faulty=fm, order=oc, first_trial=64 * 5,
                        engine=L.ENGINE_FUSED)
        finally:
            e.close()
        same(res.decisions, od, f"decisions n={n} cap={cap}")
        same(res.outcome, oo, f"outcome n={n} cap={cap}")
        assert {k: res.counters[k] for k in ocnt} == ocnt, (n, cap)


def test_om4w_staged_unchanged(engine):
    """k_om4w (n=13, m=4) includes the same headers (Philox groups, leaf blocks,
    epilogue, the one-counter fold): it must not have moved."""
    from ba_amd import lib as L
    kw = dict(seed=0x4A11, faulty_mode=L.FAULTY_RANDOM, f=4, order_mode=L.ORDER_RANDOM,
              first_trial=64 * 21)
    B = 64 * 5 * 3 + 9
    od, oo, ocnt = oracle_c.run(13, 4, B, **kw)
    dec, out, cnt = run_staged(engine, 13, 4, B, kw)
    same(dec, od, "decisions")
    same(out, oo, "outcome")
    assert cnt == list(ocnt.values())


def test_cascade_n16_m5_three_instances(engine):
    """The cascade kernels (n=16, m=5) share the Philox group code."""
    from ba_amd import lib as L
    kw = dict(seed=99, faulty_mode=L.FAULTY_RANDOM, f=5, order_mode=L.ORDER_RANDOM, first_trial=64 * 2)
    od, oo, ocnt = oracle_c.run(16, 5, 3, **kw)
    res = engine.run(16, 5, 3, engine=L.ENGINE_LEVELS, **kw)
    same(res.decisions, od, "decisions")
    same(res.outcome, oo, "outcome")
    assert {k: res.counters[k] for k in ocnt} == ocnt
