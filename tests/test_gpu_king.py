"""GPU tests of Phase King (docs/SEMANTICS.md §9): k_king through the C ABI against
the message-form reference model (tests/king_model.py).  Every comparison is exact:
decisions, outcome bytes, settled bytes and all 12 run counters."""
import ctypes
import functools
import itertools

import numpy as np
import pytest

import ba_oracle as O
import king_model as K

pytestmark = pytest.mark.gpu

# (1,0), (2,1): degenerate; (3,5): m > n-1; (4,1): n = 4m; (8,2): the even-n tie;
# (13,3): odd n, a sender pair with one sender; (17,4): a second group of sender
# pairs; (31,7), (32,7): the last lanes; (32,8): nine phases, the largest everything
SHAPES = [(1, 0), (2, 1), (3, 5), (4, 1), (5, 1), (8, 2), (9, 2), (10, 3), (13, 3), (17, 4),
          (31, 7), (32, 7), (32, 8)]
SEEDS = [0xBA5EED, 0x5157ED0123456789]
POLICIES = [K.KING_COIN, K.KING_SPLIT]
B = 229  # three full words and a partial one


def arrays(ref):
    dec, out, stl, cnt = ref
    return np.array(dec, np.uint64), np.array(out, np.uint8), np.array(stl, np.uint8), cnt


@functools.lru_cache(maxsize=None)
def model(n, m, policy, batch, seed, faulty_mode, f, order_mode, first_trial=0):
    """Reference results of a run that draws its own inputs (computed once, shared)."""
    return arrays(K.run(n, m, policy, seed=seed, faulty_mode=faulty_mode, f=f, order_mode=order_mode,
                        first_trial=first_trial, batch=batch))


def same(a, b, what):
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape, f"{what}: shape {a.shape} != {b.shape}"
    if not np.array_equal(a, b):
        idx = np.nonzero(a != b)[0]
        raise AssertionError(f"{what}: {len(idx)} mismatches, first at {idx[:5].tolist()}: "
                             f"got {a[idx[:5]].tolist()} want {b[idx[:5]].tolist()}")


def check(res, ref, what):
    dec, out, stl, cnt = ref
    same(res.decisions, dec, f"{what} decisions")
    same(res.outcome, out, f"{what} outcome")
    same(res.settled, stl, f"{what} settled")
    assert len(cnt) == 12
    assert {k: res.counters[k] for k in cnt} == cnt, what


@pytest.mark.parametrize("policy", POLICIES)
@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("n,m", SHAPES)
def test_shapes_bit_exact(engine, n, m, seed, policy):
    from ba_amd import lib as L
    res = engine.run_king(n, m, B, policy, seed=seed, faulty_mode=L.FAULTY_RANDOM, f=n,
                          order_mode=L.ORDER_RANDOM, want_settled=True)
    check(res, model(n, m, policy, B, seed, O.FAULTY_RANDOM, n, O.ORDER_RANDOM), f"n={n} m={m}")
    assert res.counters["undefined_decisions"] == 0


SINK_B = 64 * 68 + 37  # 69 words: 18 four-wave blocks, 72 reporting waves > the sink's 64 replicas


@pytest.mark.parametrize("policy", POLICIES)
@pytest.mark.parametrize("n,m", [(10, 3), (5, 1)])
def test_sink_path_bit_exact(engine, n, m, policy):
    """A launch of more than 64 reporting waves adds its counters through the sink's
    replicas (sink_counters, ba_device.hpp), where the smaller batches here add
    straight into the caller's: the whole batch against the model through the host
    entry, then as two device calls accumulating into one d_counters, then twice
    whole through the device entry (the first launch must leave the replicas zero).
    (5, 1) is the smallest shape inside Phase King's bound n > 4m."""
    import torch
    from ba_amd import lib as L
    words = (SINK_B + 63) // 64
    assert 4 * ((words + 3) // 4) > 64  # launch_king: one unit per wave, four-wave blocks
    first = 64 * 9
    kw = dict(seed=SEEDS[0], faulty_mode=L.FAULTY_RANDOM, f=n, order_mode=L.ORDER_RANDOM)
    ref = model(n, m, policy, SINK_B, SEEDS[0], O.FAULTY_RANDOM, n, O.ORDER_RANDOM, first)
    check(engine.run_king(n, m, SINK_B, policy, first_trial=first, want_settled=True, **kw), ref,
          f"host n={n} m={m} policy={policy}")
    s = torch.cuda.current_stream().cuda_stream
    half = 64 * 34
    for what, calls, times in (("two halves", ((0, half), (half, SINK_B - half)), 1),
                               ("whole twice", ((0, SINK_B), (0, SINK_B)), 2)):
        dec = torch.full((SINK_B,), -1, dtype=torch.int64, device="cuda")
        out = torch.full((SINK_B,), 254, dtype=torch.uint8, device="cuda")
        stl = torch.full((SINK_B,), 254, dtype=torch.uint8, device="cuda")
        cnt = torch.zeros(16, dtype=torch.int64, device="cuda")
        for t0, count in calls:
            engine.run_king_device(L.make_params(n, m, first_trial=first + t0, **kw), count, policy,
                                   d_decisions=dec[t0:].data_ptr(), d_outcome=out[t0:].data_ptr(),
                                   d_settled=stl[t0:].data_ptr(), d_counters=cnt.data_ptr(), stream=s)
        torch.cuda.synchronize()
        same(dec.cpu().numpy().view(np.uint64), ref[0], f"{what} decisions")
        same(out.cpu().numpy(), ref[1], f"{what} outcome")
        same(stl.cpu().numpy(), ref[2], f"{what} settled")
        got = cnt.cpu().tolist()
        assert dict(zip(L.COUNTER_NAMES, got)) == {k: times * v for k, v in ref[3].items()}, what
        assert got[12:] == [0, 0, 0, 0]


@pytest.mark.parametrize("policy", POLICIES)
@pytest.mark.parametrize("first", [0, 64 * 5, 1 << 38])
def test_first_trial(engine, first, policy):
    from ba_amd import lib as L
    res = engine.run_king(10, 3, B, policy, seed=SEEDS[0], faulty_mode=L.FAULTY_RANDOM, f=10,
                          order_mode=L.ORDER_RANDOM, first_trial=first, want_settled=True)
    check(res, model(10, 3, policy, B, SEEDS[0], O.FAULTY_RANDOM, 10, O.ORDER_RANDOM, first),
          f"first={first}")


@pytest.mark.parametrize("policy", POLICIES)
@pytest.mark.parametrize("n,m", [(5, 1), (10, 3), (32, 7)])
def test_given_inputs(engine, n, m, policy):
    """No traitor, every general faulty, a faulty commander only, mask bits at and
    above n (ignored), and every order code, BA_OTHER included."""
    full = (1 << n) - 1
    high = (0xFFFFFFFF & ~full) if n < 32 else 0
    masks = [0, full, 1, high, high | 1, high | full, 0b110 & full, full & ~1]
    rows = [(fm, oc) for fm in masks for oc in (0, 1, 2)]
    rows = rows * 4  # 96 trials: two words, the coins differ per trial
    fm = np.array([r[0] for r in rows], np.uint32)
    oc = np.array([r[1] for r in rows], np.uint8)
    res = engine.run_king(n, m, len(rows), policy, seed=99, faulty=fm, order=oc, first_trial=128,
                          want_settled=True)
    ref = K.run(n, m, policy, seed=99, faulty=fm.tolist(), order=oc.tolist(), first_trial=128,
                batch=len(rows))
    check(res, arrays(ref), f"given n={n} m={m}")
    # a loyal commander within the bound (|F| <= m and n > 4m; (10, 3) is outside,
    # so only its traitor-free rows count): every loyal lieutenant decides the order,
    # and the loyal generals agree from round 0 on
    lts = (1 << (2 * (n - 1))) - 1
    seen = 0
    for i, (f_, o_) in enumerate(rows):
        f_ &= full
        if not f_ & 1 and bin(f_).count("1") <= (m if n > 4 * m else 0):
            loyal = sum(3 << (2 * (r - 1)) for r in range(1, n) if not (f_ >> r) & 1)
            want = (0x5555555555555555 if o_ == 1 else 0) & lts
            assert int(res.decisions[i]) & loyal == want & loyal, (i, f_, o_)
            assert int(res.settled[i]) == 0, (i, f_, o_)
            seen += 1
    assert seen >= 24


def test_sharding_and_device_accumulation(engine):
    import torch
    from ba_amd import lib as L
    kw = dict(seed=SEEDS[1], faulty_mode=L.FAULTY_RANDOM, f=10, order_mode=L.ORDER_RANDOM)
    for policy in POLICIES:
        whole = engine.run_king(10, 3, 256, policy, want_settled=True, **kw)
        a = engine.run_king(10, 3, 128, policy, want_settled=True, **kw)
        b = engine.run_king(10, 3, 128, policy, first_trial=128, want_settled=True, **kw)
        same(np.concatenate([a.decisions, b.decisions]), whole.decisions, "decisions")
        same(np.concatenate([a.outcome, b.outcome]), whole.outcome, "outcome")
        same(np.concatenate([a.settled, b.settled]), whole.settled, "settled")
        assert {k: a.counters[k] + b.counters[k] for k in a.counters} == whole.counters
        check(whole, model(10, 3, policy, 256, SEEDS[1], O.FAULTY_RANDOM, 10, O.ORDER_RANDOM), "whole")
        # the device entry accumulates into d_counters across calls
        cnt = torch.zeros(16, dtype=torch.int64, device="cuda")
        s = torch.cuda.current_stream().cuda_stream
        for first in (0, 128):
            engine.run_king_device(L.make_params(10, 3, first_trial=first, **kw), 128, policy,
                                   d_counters=cnt.data_ptr(), stream=s)
        torch.cuda.synchronize()
        got = dict(zip(L.COUNTER_NAMES, cnt.cpu().tolist()))
        assert got == whole.counters
        assert cnt.cpu().tolist()[12:] == [0, 0, 0, 0]


def test_host_entry_chunks(engine, monkeypatch):
    """The host entry's chunk loop (forced small): same bits as one chunk."""
    from ba_amd import lib as L
    kw = dict(seed=SEEDS[0], faulty_mode=L.FAULTY_RANDOM, f=10, order_mode=L.ORDER_RANDOM)
    rng = np.random.default_rng(1)
    fm = rng.integers(0, 1 << 10, B, dtype=np.uint64).astype(np.uint32)
    oc = rng.choice([0, 1, 2], B).astype(np.uint8)
    one = engine.run_king(10, 3, B, K.KING_COIN, want_settled=True, **kw)
    one_g = engine.run_king(10, 3, B, K.KING_SPLIT, seed=3, faulty=fm, order=oc, want_settled=True)
    monkeypatch.setenv("BA_KING_HOST_CHUNK", "64")
    for ref, res in ((one, engine.run_king(10, 3, B, K.KING_COIN, want_settled=True, **kw)),
                     (one_g, engine.run_king(10, 3, B, K.KING_SPLIT, seed=3, faulty=fm, order=oc,
                                             want_settled=True))):
        same(res.decisions, ref.decisions, "decisions")
        same(res.outcome, ref.outcome, "outcome")
        same(res.settled, ref.settled, "settled")
        assert res.counters == ref.counters
    check(one, model(10, 3, K.KING_COIN, B, SEEDS[0], O.FAULTY_RANDOM, 10, O.ORDER_RANDOM), "one chunk")


def test_host_entry_settled_without_outcome(engine, monkeypatch):
    """The extra plane alone through the chunked host entry: `settled` rides behind the
    outcome bytes in one staging buffer and is asked for without them (64-trial chunks,
    a partial last word)."""
    from ba_amd import lib as L
    n, m, b = 4, 1, 130
    monkeypatch.setenv("BA_KING_HOST_CHUNK", "64")
    res = engine.run_king(n, m, b, K.KING_COIN, seed=SEEDS[0], faulty_mode=L.FAULTY_RANDOM, f=n,
                          order_mode=L.ORDER_RANDOM, want_decisions=False, want_outcome=False,
                          want_settled=True)
    ref = model(n, m, K.KING_COIN, b, SEEDS[0], O.FAULTY_RANDOM, n, O.ORDER_RANDOM)
    assert res.decisions is None and res.outcome is None
    same(res.settled, ref[2], "settled")
    assert {k: res.counters[k] for k in ref[3]} == ref[3]


def test_staged_inputs_equal_in_kernel_draws_and_optional_outputs(engine):
    """ba_gen_inputs_device + GIVEN == drawing in the kernel; the decisions, outcome
    and settled pointers are each optional, in every combination, and an absent
    buffer is not touched."""
    import torch
    from ba_amd import lib as L
    n, m = 10, 3
    kw = dict(seed=SEEDS[0], faulty_mode=L.FAULTY_RANDOM, f=n, order_mode=L.ORDER_RANDOM)
    ref = model(n, m, K.KING_COIN, B, SEEDS[0], O.FAULTY_RANDOM, n, O.ORDER_RANDOM)
    s = torch.cuda.current_stream().cuda_stream
    fm = torch.zeros(B, dtype=torch.int32, device="cuda")
    oc = torch.zeros(B, dtype=torch.uint8, device="cuda")
    engine.gen_inputs_device(L.make_params(n, m, **kw), B, d_faulty=fm.data_ptr(), d_order=oc.data_ptr(),
                             stream=s)
    given = L.make_params(n, m, seed=SEEDS[0])
    drawn = L.make_params(n, m, **kw)
    for p, ins in ((given, dict(d_faulty=fm.data_ptr(), d_order=oc.data_ptr())), (drawn, {})):
        for wd, wo, ws in itertools.product((False, True), repeat=3):
            dec = torch.full((B,), -1, dtype=torch.int64, device="cuda")
            out = torch.full((B,), 254, dtype=torch.uint8, device="cuda")
            stl = torch.full((B,), 254, dtype=torch.uint8, device="cuda")
            cnt = torch.zeros(16, dtype=torch.int64, device="cuda")
            engine.run_king_device(p, B, K.KING_COIN, d_decisions=dec.data_ptr() if wd else 0,
                                   d_outcome=out.data_ptr() if wo else 0,
                                   d_settled=stl.data_ptr() if ws else 0, d_counters=cnt.data_ptr(),
                                   stream=s, **ins)
            torch.cuda.synchronize()
            what = f"given={p is given} dec={wd} out={wo} settled={ws}"
            same(dec.cpu().numpy().view(np.uint64), ref[0] if wd else np.full(B, 2**64 - 1, np.uint64),
                 what + " decisions")
            same(out.cpu().numpy(), ref[1] if wo else np.full(B, 254, np.uint8), what + " outcome")
            same(stl.cpu().numpy(), ref[2] if ws else np.full(B, 254, np.uint8), what + " settled")
            assert dict(zip(L.COUNTER_NAMES, cnt.cpu().tolist())) == ref[3], what


def test_theory_counters(engine):
    """The theorem on counters alone, 65,536 trials each: n > 4m and f <= m never
    break IC1 or IC2 under either policy; f > m can."""
    from ba_amd import lib as L
    T = 65536
    kw = dict(seed=2024, order_mode=L.ORDER_RANDOM, want_decisions=False, want_outcome=False)
    for policy in POLICIES:
        for n, m in ((9, 2), (32, 7)):
            c = engine.run_king(n, m, T, policy, faulty_mode=L.FAULTY_RANDOM, f=m, **kw).counters
            assert c["trials"] == T and c["in_bound"] == T
            assert c["bound_violations"] == 0 and c["agreement"] == T
            assert c["validity"] == c["validity_applicable"]
            assert c["undefined_decisions"] == 0
    c = engine.run_king(5, 1, T, K.KING_SPLIT, faulty_mode=L.FAULTY_EXACT, f=2, **kw).counters
    assert c["trials"] == T and c["in_bound"] == 0 and c["bound_violations"] == 0
    assert c["agreement"] < T
    assert c["undefined_decisions"] == 0 and c["faulty_total"] == 2 * T


def test_errors(engine):
    from ba_amd import lib as L
    kw = dict(faulty_mode=L.FAULTY_EXACT, f=0, order_mode=L.ORDER_CONST)

    def code(**over):
        a = dict(n=5, m=1, batch=64, policy=K.KING_COIN)
        a.update(kw)
        a.update(over)
        with pytest.raises(L.BAError) as e:
            engine.run_king(a.pop("n"), a.pop("m"), a.pop("batch"), a.pop("policy"), **a)
        return e.value.code

    assert code(lie_mode=L.LIE_TABLE) == L.ENOTSUP
    assert code(n=0) == L.EINVAL
    assert code(n=33) == L.EINVAL
    assert code(m=9) == L.EINVAL
    assert code(policy=2) == L.EINVAL
    assert code(first_trial=32) == L.EINVAL
    assert code(faulty_mode=L.FAULTY_GIVEN) == L.EINVAL  # no faulty_mask
    assert code(order_mode=L.ORDER_GIVEN) == L.EINVAL    # no order
    for eng in (L.ENGINE_FUSED, L.ENGINE_LEVELS):
        assert code(engine=eng) == L.EINVAL
        assert b"engine" in engine.lib.ba_last_error()
    # the trial index may not wrap: the last trial is at most 2^64 - 1
    with pytest.raises(L.BAError) as e:
        engine.run_king(5, 1, 65, first_trial=2**64 - 64, **kw)
    assert e.value.code == L.EINVAL and "first_trial" in str(e.value)
    kr = dict(seed=5, faulty_mode=L.FAULTY_RANDOM, f=5, order_mode=L.ORDER_RANDOM)
    top = engine.run_king(5, 1, 64, first_trial=2**64 - 64, want_settled=True, **kr)  # ends at 2^64
    check(top, arrays(K.run(5, 1, first_trial=2**64 - 64, batch=64, **kr)), "top")
    # batch = 0: BA_OK with zero counters
    res = engine.run_king(5, 1, 0, **kw)
    assert all(v == 0 for v in res.counters.values())
    # a NULL ctx and NULL params are errors, not crashes
    cnt = L.Counters()
    assert engine.lib.ba_king_run_trials(engine.handle, None, 0, 64, None, None, None, None, None,
                                         ctypes.byref(cnt)) == L.EINVAL
    # the ctx still works
    assert engine.run_king(5, 1, 64, **kw).counters["trials"] == 64


def test_bench_size_equals_sum_of_sixteen(engine):
    """1,048,576 trials at (10, 3) in one call == sixteen 65,536-trial calls:
    the persistent word loop and the counter sink at bench size."""
    from ba_amd import lib as L
    kw = dict(seed=0xBA5EED, faulty_mode=L.FAULTY_RANDOM, f=3, order_mode=L.ORDER_RANDOM,
              want_decisions=False, want_outcome=False)
    T, Kc = 1 << 20, 16
    whole = engine.run_king(10, 3, T, K.KING_COIN, **kw).counters
    tot = dict.fromkeys(whole, 0)
    for i in range(Kc):
        c = engine.run_king(10, 3, T // Kc, K.KING_COIN, first_trial=i * (T // Kc), **kw).counters
        for k in tot:
            tot[k] += c[k]
    assert whole == tot
    assert whole["trials"] == T
