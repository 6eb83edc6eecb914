"""GPU tests of RAND against the stalling adversary (docs/SEMANTICS.md §15): k_rstall
through the C ABI against the reference model (tests/rstall_model.py), which runs every
phase.  Every comparison is exact: decisions, outcome bytes, decided bytes and all 12
run counters.  No test asserts a statistical rate."""
import ctypes
import functools
import itertools

import numpy as np
import pytest

import ba_oracle as O
import renum_model as RN
import rstall_model as SM

pytestmark = pytest.mark.gpu

# test_gpu_rand.py's shapes: degenerate ones, thresholds beyond n, n = 3m, n <= 2m, odd
# n, the last mask bits and m = 0.  f and the traitors' ranks differ per trial of a word.
SHAPES = [(1, 0), (2, 1), (3, 5), (4, 1), (6, 2), (5, 3), (7, 2), (10, 3), (13, 4), (17, 5),
          (31, 10), (32, 10), (32, 0)]
SEEDS = [0xBA5EED, 0x5157ED0123456789]
COINS = [SM.RAND_LOCAL, SM.RAND_COMMON]
B = 229  # three full words and a partial one


def arrays(ref):
    dec, out, dcd, cnt = ref
    return np.array(dec, np.uint64), np.array(out, np.uint8), np.array(dcd, np.uint8), cnt


@functools.lru_cache(maxsize=None)
def model(n, m, R, coin, batch, seed, faulty_mode, f, order_mode, first_trial=0):
    """Reference results of a run that draws its own inputs (computed once, shared).  Up
    to eight phases the message form; beyond, the plane form, which
    tests/test_rstall_model.py holds equal to it and which draws 64 trials' coins at once."""
    return arrays(SM.run(n, m, R, coin, seed=seed, faulty_mode=faulty_mode, f=f, order_mode=order_mode,
                         first_trial=first_trial, batch=batch, form="message" if R <= 8 else "plane"))


def same(a, b, what):
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape, f"{what}: shape {a.shape} != {b.shape}"
    if not np.array_equal(a, b):
        idx = np.nonzero(a != b)[0]
        raise AssertionError(f"{what}: {len(idx)} mismatches, first at {idx[:5].tolist()}: "
                             f"got {a[idx[:5]].tolist()} want {b[idx[:5]].tolist()}")


def check(res, ref, what):
    dec, out, dcd, cnt = ref
    same(res.decisions, dec, f"{what} decisions")
    same(res.outcome, out, f"{what} outcome")
    same(res.decided, dcd, f"{what} decided")
    assert len(cnt) == 12
    assert {k: res.counters[k] for k in cnt} == cnt, what


@pytest.mark.parametrize("R", [1, 3])
@pytest.mark.parametrize("coin", COINS)
@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("n,m", SHAPES)
def test_shapes_bit_exact(engine, n, m, seed, coin, R):
    from ba_amd import lib as L
    res = engine.run_rstall(n, m, B, R, coin, seed=seed, faulty_mode=L.FAULTY_RANDOM, f=n,
                            order_mode=L.ORDER_RANDOM, want_decided=True)
    check(res, model(n, m, R, coin, B, seed, O.FAULTY_RANDOM, n, O.ORDER_RANDOM), f"n={n} m={m} R={R}")
    assert res.counters["undefined_decisions"] == 0


@pytest.mark.parametrize("coin", COINS)
@pytest.mark.parametrize("exact", [True, False])
@pytest.mark.parametrize("R", [24, 250])
@pytest.mark.parametrize("n,m", [(4, 1), (10, 3)])
def test_long_runs_and_the_early_finish(engine, n, m, R, exact, coin):
    """FAULTY_EXACT f = m: every word is in bound, and the kernel skips a word's phases
    once all n generals have decided; under the local coin some trials stall for many
    phases first.  FAULTY_RANDOM f = n: in-bound and out-of-bound trials share words,
    which then run every phase.  Both equal the model, which always runs all R (Philox
    tags up to 256 + 750 at R = 250)."""
    from ba_amd import lib as L
    mode, f = (L.FAULTY_EXACT, m) if exact else (L.FAULTY_RANDOM, n)
    res = engine.run_rstall(n, m, B, R, coin, seed=SEEDS[0], faulty_mode=mode, f=f,
                            order_mode=L.ORDER_RANDOM, want_decided=True)
    ref = model(n, m, R, coin, B, SEEDS[0], mode, f, O.ORDER_RANDOM)
    check(res, ref, f"n={n} m={m} R={R} exact={exact}")
    if exact:
        assert res.counters["in_bound"] == B and SM.UNSAFE not in ref[2]
    else:
        assert 0 < res.counters["in_bound"] < B
    # without the decided output the kernel takes the early finish from D alone
    bare = engine.run_rstall(n, m, B, R, coin, seed=SEEDS[0], faulty_mode=mode, f=f,
                             order_mode=L.ORDER_RANDOM)
    assert bare.decided is None
    same(bare.decisions, ref[0], "decisions, no decided output")
    same(bare.outcome, ref[1], "outcome, no decided output")
    assert {k: bare.counters[k] for k in ref[3]} == ref[3]


@pytest.mark.parametrize("coin", COINS)
@pytest.mark.parametrize("first", [0, 320, 1 << 38])
def test_first_trial(engine, first, coin):
    from ba_amd import lib as L
    res = engine.run_rstall(10, 3, B, 3, coin, seed=SEEDS[0], faulty_mode=L.FAULTY_RANDOM, f=10,
                            order_mode=L.ORDER_RANDOM, first_trial=first, want_decided=True)
    check(res, model(10, 3, 3, coin, B, SEEDS[0], O.FAULTY_RANDOM, 10, O.ORDER_RANDOM, first),
          f"first={first}")


@pytest.mark.parametrize("coin", COINS)
def test_given_inputs(engine, coin):
    """(4,1): every faulty set of one and of two generals, both orders, 96 trials, so one
    word holds every set; in bound the trial is never unsafe, and with a loyal commander
    everyone decides its order in phase 1."""
    n, m, R = 4, 1, 6
    sets = [sum(1 << g for g in c) for k in (1, 2) for c in itertools.combinations(range(n), k)]
    rows = [(fm, oc) for fm in sets for oc in (0, 1)] * 5
    rows = rows[:96]
    fm = np.array([r[0] for r in rows], np.uint32)
    oc = np.array([r[1] for r in rows], np.uint8)
    res = engine.run_rstall(n, m, len(rows), R, coin, seed=99, faulty=fm, order=oc, first_trial=128,
                            want_decided=True)
    ref = SM.run(n, m, R, coin, seed=99, faulty=fm.tolist(), order=oc.tolist(), first_trial=128,
                 batch=len(rows))
    check(res, arrays(ref), "given (4,1)")
    for i, (f_, o_) in enumerate(rows):
        if bin(f_).count("1") <= m:
            assert int(res.decided[i]) != SM.UNSAFE, (i, f_, o_)
            if not f_ & 1:
                loyal = sum(3 << (2 * (r - 1)) for r in range(1, n) if not (f_ >> r) & 1)
                assert int(res.decisions[i]) & loyal == (0x55 if o_ == 1 else 0) & loyal, (i, f_, o_)
                assert int(res.decided[i]) == 1, (i, f_, o_)


@pytest.mark.parametrize("coin", COINS)
def test_device_entry(engine, coin):
    """On a stream of its own: two calls accumulate d_counters to twice one call's
    totals, d_decided is optional and an absent buffer is not touched."""
    import torch
    from ba_amd import lib as L
    n, m, R = 10, 3, 3
    kw = dict(seed=SEEDS[1], faulty_mode=L.FAULTY_RANDOM, f=n, order_mode=L.ORDER_RANDOM)
    ref = model(n, m, R, coin, B, SEEDS[1], O.FAULTY_RANDOM, n, O.ORDER_RANDOM)
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        dec = torch.full((B,), -1, dtype=torch.int64, device="cuda")
        out = torch.full((B,), 253, dtype=torch.uint8, device="cuda")
        dcd = torch.full((B,), 253, dtype=torch.uint8, device="cuda")
        cnt = torch.zeros(16, dtype=torch.int64, device="cuda")
        for want in (True, False):
            engine.run_rstall_device(L.make_params(n, m, **kw), B, R, coin, d_decisions=dec.data_ptr(),
                                     d_outcome=out.data_ptr(), d_decided=dcd.data_ptr() if want else 0,
                                     d_counters=cnt.data_ptr(), stream=stream.cuda_stream)
    stream.synchronize()
    same(dec.cpu().numpy().view(np.uint64), ref[0], "decisions")
    same(out.cpu().numpy(), ref[1], "outcome")
    same(dcd.cpu().numpy(), ref[2], "decided")
    got = cnt.cpu().tolist()
    assert dict(zip(L.COUNTER_NAMES, got)) == {k: 2 * v for k, v in ref[3].items()}
    assert got[12:] == [0, 0, 0, 0]
    # no decided buffer at all: it stays as it was
    with torch.cuda.stream(stream):
        dcd.fill_(253)
        engine.run_rstall_device(L.make_params(n, m, **kw), B, R, coin, d_decisions=dec.data_ptr(),
                                 d_counters=cnt.data_ptr(), stream=stream.cuda_stream)
    stream.synchronize()
    same(dcd.cpu().numpy(), np.full(B, 253, np.uint8), "decided untouched")


SINK_B = 64 * 68 + 37  # 69 words: 72 reporting waves > the counter sink's 64 replicas


@pytest.mark.parametrize("coin", COINS)
def test_sink_path_and_host_chunks(engine, coin, monkeypatch):
    """A launch of more than 64 reporting waves adds its counters through the sink's
    replicas; the host entry's chunk loop (forced to 64) gives the same bits."""
    from ba_amd import lib as L
    n, m, R, first = 10, 3, 2, 64 * 9
    kw = dict(seed=SEEDS[0], faulty_mode=L.FAULTY_RANDOM, f=n, order_mode=L.ORDER_RANDOM)
    ref = model(n, m, R, coin, SINK_B, SEEDS[0], O.FAULTY_RANDOM, n, O.ORDER_RANDOM, first)
    check(engine.run_rstall(n, m, SINK_B, R, coin, first_trial=first, want_decided=True, **kw), ref, "whole")
    monkeypatch.setenv("BA_RSTALL_HOST_CHUNK", "64")
    check(engine.run_rstall(n, m, SINK_B, R, coin, first_trial=first, want_decided=True, **kw), ref, "chunks")


@pytest.mark.parametrize("coin", COINS)
@pytest.mark.parametrize("fmask", [0b0001, 0b0010])
def test_a_trial_is_a_strategy_of_renum(engine, fmask, coin):
    """(4,1), R = 3, 16 trials: k_renum at stall_strategy's S gives the loyal lieutenants'
    decisions, the IC1 / IC2 flags and the decided byte of the k_rstall trial.  A faulty
    lieutenant's own decision is not compared: its toss is dead there and drawn here."""
    from ba_amd import lib as L
    n, m, R, seed = 4, 1, 3, SEEDS[0]
    orders = [L.ATTACK if t & 1 else L.RETREAT for t in range(16)]
    res = engine.run_rstall(n, m, 16, R, coin, seed=seed, faulty=np.full(16, fmask, np.uint32),
                            order=np.array(orders, np.uint8), want_decided=True)
    loyal = sum(3 << (2 * (r - 1)) for r in range(1, n) if not (fmask >> r) & 1)
    for t, order in enumerate(orders):
        S = SM.stall_strategy(coin, n, m, R, fmask, int(order == L.ATTACK), seed, t)
        ren = engine.run_renum(coin, n, m, R, fmask, order, first=S & ~63, count=64, want_decisions=True,
                               want_outcome=True, want_decided=True)
        k = S & 63
        assert int(ren.decisions[k]) & loyal == int(res.decisions[t]) & loyal, (t, S)
        assert int(ren.outcome[k]) & 0x3C == int(res.outcome[t]) & 0x3C, (t, S)
        assert int(ren.decided[k]) == int(res.decided[t]), (t, S)
    assert RN.bits_formula(coin, n, m, R, fmask) <= 39


def test_errors(engine):
    from ba_amd import lib as L
    kw = dict(faulty_mode=L.FAULTY_EXACT, f=0, order_mode=L.ORDER_CONST)

    def code(**over):
        a = dict(n=4, m=1, batch=64, phases=2, coin=SM.RAND_COMMON)
        a.update(kw)
        a.update(over)
        with pytest.raises(L.BAError) as e:
            engine.run_rstall(a.pop("n"), a.pop("m"), a.pop("batch"), a.pop("phases"), a.pop("coin"), **a)
        return e.value.code

    assert code(lie_mode=L.LIE_TABLE) == L.ENOTSUP
    assert code(n=0) == L.EINVAL
    assert code(n=33) == L.EINVAL
    assert code(n=32, m=11) == L.EINVAL
    assert engine.run_rstall(32, 10, 64, 1, **kw).counters["trials"] == 64  # m = 10 is accepted
    assert code(coin=2) == L.EINVAL
    assert code(phases=0) == L.EINVAL
    assert code(phases=251) == L.EINVAL
    assert L.RSTALL_MAX_PHASES == 250
    assert engine.run_rstall(4, 1, 64, 250, **kw).counters["trials"] == 64  # R = 250 is accepted
    assert code(first_trial=32) == L.EINVAL
    assert code(faulty_mode=L.FAULTY_GIVEN) == L.EINVAL  # no faulty_mask
    assert code(order_mode=L.ORDER_GIVEN) == L.EINVAL    # no order
    for eng in (L.ENGINE_FUSED, L.ENGINE_LEVELS):
        assert code(engine=eng) == L.EINVAL
        assert b"engine" in engine.lib.ba_last_error()
    # the device entry validates alike, and needs d_counters
    with pytest.raises(L.BAError) as e:
        engine.run_rstall_device(L.make_params(4, 1, **kw), 64, 251)
    assert e.value.code == L.EINVAL
    with pytest.raises(L.BAError) as e:
        engine.run_rstall_device(L.make_params(4, 1, **kw), 64, 2)
    assert e.value.code == L.EINVAL and "d_counters" in str(e.value)
    # batch = 0: BA_OK with zero counters
    res = engine.run_rstall(4, 1, 0, 2, **kw)
    assert all(v == 0 for v in res.counters.values())
    # NULL ctx and NULL params are errors, not crashes
    cnt = L.Counters()
    p = L.make_params(4, 1, **kw)
    assert engine.lib.ba_rstall_run_trials(None, ctypes.byref(p), 1, 2, 64, None, None, None, None, None,
                                           ctypes.byref(cnt)) == L.EINVAL
    assert engine.lib.ba_rstall_run_trials(engine.handle, None, 1, 2, 64, None, None, None, None, None,
                                           ctypes.byref(cnt)) == L.EINVAL
    # the ctx still works
    assert engine.run_rstall(4, 1, 64, 2, **kw).counters["trials"] == 64


def test_coin_calls():
    from ba_amd import lib as L
    for n, R, coin in itertools.product((1, 4, 10, 32), (1, 16, 250), COINS):
        assert L.rstall_coin_calls(n, R, coin) == R * (n if coin == L.RAND_LOCAL else 1)
        assert L.rstall_coin_calls(n, R, coin) == SM.coin_calls(n, R, coin)
    for bad in ((0, 1, 0), (33, 1, 0), (4, 0, 0), (4, 251, 0), (4, 1, 2)):
        assert L.rstall_coin_calls(*bad) == 0
