"""GPU tests of randomized agreement (docs/SEMANTICS.md §13): k_rand through the C ABI
against the reference model (tests/rand_model.py), which runs every phase.  Every
comparison is exact: decisions, outcome bytes, decided bytes and all 12 run
counters.  No test asserts a statistical rate."""
import ctypes
import functools
import itertools

import numpy as np
import pytest

import ba_oracle as O
import rand_model as RM

pytestmark = pytest.mark.gpu

# (1,0), (2,1): degenerate; (3,5): thresholds beyond n, nobody ever proposes; (4,1):
# the smallest n > 3m; (6,2): n = 3m; (5,3): n <= 2m; (13,4): odd n, a sender pair with
# one sender; (17,5): a second group of sender pairs; (31,10), (32,10): the last lanes,
# thresholds 21 / 22 and 11; (32,0): threshold 17 and 1, one plane short of the top
SHAPES = [(1, 0), (2, 1), (3, 5), (4, 1), (6, 2), (5, 3), (7, 2), (10, 3), (13, 4), (17, 5),
          (31, 10), (32, 10), (32, 0)]
SEEDS = [0xBA5EED, 0x5157ED0123456789]
POLICIES = [RM.KING_COIN, RM.KING_SPLIT]
COINS = [RM.RAND_LOCAL, RM.RAND_COMMON]
B = 229  # three full words and a partial one


def arrays(ref):
    dec, out, dcd, cnt = ref
    return np.array(dec, np.uint64), np.array(out, np.uint8), np.array(dcd, np.uint8), cnt


@functools.lru_cache(maxsize=None)
def model(n, m, R, policy, coin, batch, seed, faulty_mode, f, order_mode, first_trial=0):
    """Reference results of a run that draws its own inputs (computed once, shared).
    Up to eight phases the message form; beyond, the plane form, which
    tests/test_rand_model.py holds equal to it and which draws 64 trials' coins at once."""
    return arrays(RM.run(n, m, R, policy, coin, seed=seed, faulty_mode=faulty_mode, f=f,
                         order_mode=order_mode, first_trial=first_trial, batch=batch,
                         form="message" if R <= 8 else "plane"))


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
@pytest.mark.parametrize("policy", POLICIES)
@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("n,m", SHAPES)
def test_shapes_bit_exact(engine, n, m, seed, policy, coin, R):
    from ba_amd import lib as L
    res = engine.run_rand(n, m, B, R, policy, coin, seed=seed, faulty_mode=L.FAULTY_RANDOM, f=n,
                          order_mode=L.ORDER_RANDOM, want_decided=True)
    check(res, model(n, m, R, policy, coin, B, seed, O.FAULTY_RANDOM, n, O.ORDER_RANDOM),
          f"n={n} m={m} R={R}")
    assert res.counters["undefined_decisions"] == 0


@pytest.mark.parametrize("coin", COINS)
@pytest.mark.parametrize("policy", POLICIES)
@pytest.mark.parametrize("exact", [True, False])
@pytest.mark.parametrize("n,m", [(4, 1), (10, 3)])
def test_early_finish_is_invisible(engine, n, m, exact, policy, coin):
    """R = 24.  FAULTY_EXACT f = m: every word is in bound, and the kernel skips a
    word's phases once all n generals have decided.  FAULTY_RANDOM f = n: in-bound and
    out-of-bound trials share words, which then run every phase.  Both equal the model,
    which always runs all 24."""
    from ba_amd import lib as L
    mode, f = (L.FAULTY_EXACT, m) if exact else (L.FAULTY_RANDOM, n)
    res = engine.run_rand(n, m, B, 24, policy, coin, seed=SEEDS[0], faulty_mode=mode, f=f,
                          order_mode=L.ORDER_RANDOM, want_decided=True)
    ref = model(n, m, 24, policy, coin, B, SEEDS[0], mode, f, O.ORDER_RANDOM)
    check(res, ref, f"n={n} m={m} exact={exact}")
    if exact:
        assert res.counters["in_bound"] == B and RM.UNSAFE not in ref[2]
    else:
        assert 0 < res.counters["in_bound"] < B
    # without the decided output the kernel takes the early finish from D alone
    bare = engine.run_rand(n, m, B, 24, policy, coin, seed=SEEDS[0], faulty_mode=mode, f=f,
                           order_mode=L.ORDER_RANDOM)
    same(bare.decisions, ref[0], "decisions, no decided output")
    assert {k: bare.counters[k] for k in ref[3]} == ref[3]


@pytest.mark.parametrize("coin", COINS)
@pytest.mark.parametrize("exact", [True, False])
def test_sixty_four_phases(engine, exact, coin):
    """(10,3), R = 64: Philox tags up to 256 + 192 = 448."""
    from ba_amd import lib as L
    mode, f = (L.FAULTY_EXACT, 3) if exact else (L.FAULTY_RANDOM, 10)
    res = engine.run_rand(10, 3, B, 64, RM.KING_COIN, coin, seed=SEEDS[1], faulty_mode=mode, f=f,
                          order_mode=L.ORDER_RANDOM, want_decided=True)
    check(res, model(10, 3, 64, RM.KING_COIN, coin, B, SEEDS[1], mode, f, O.ORDER_RANDOM),
          f"R=64 exact={exact}")


@pytest.mark.parametrize("coin", COINS)
@pytest.mark.parametrize("policy", POLICIES)
@pytest.mark.parametrize("first", [0, 320, 1 << 38])
def test_first_trial(engine, first, policy, coin):
    from ba_amd import lib as L
    res = engine.run_rand(10, 3, B, 3, policy, coin, seed=SEEDS[0], faulty_mode=L.FAULTY_RANDOM, f=10,
                          order_mode=L.ORDER_RANDOM, first_trial=first, want_decided=True)
    check(res, model(10, 3, 3, policy, coin, B, SEEDS[0], O.FAULTY_RANDOM, 10, O.ORDER_RANDOM, first),
          f"first={first}")


@pytest.mark.parametrize("coin", COINS)
@pytest.mark.parametrize("policy", POLICIES)
@pytest.mark.parametrize("n,m", [(4, 1), (10, 3), (32, 10)])
def test_given_inputs(engine, n, m, policy, coin):
    """No traitor, every general faulty, a faulty commander only, mask bits at and
    above n (ignored), and every order code, BA_OTHER included."""
    full = (1 << n) - 1
    high = (0xFFFFFFFF & ~full) if n < 32 else 0
    masks = [0, full, 1, high, high | 1, high | full, 0b110 & full, full & ~1]
    rows = [(fm, oc) for fm in masks for oc in (0, 1, 2)]
    rows = rows * 4  # 96 trials: two words, the coins differ per trial
    fm = np.array([r[0] for r in rows], np.uint32)
    oc = np.array([r[1] for r in rows], np.uint8)
    res = engine.run_rand(n, m, len(rows), 3, policy, coin, seed=99, faulty=fm, order=oc,
                          first_trial=128, want_decided=True)
    ref = RM.run(n, m, 3, policy, coin, seed=99, faulty=fm.tolist(), order=oc.tolist(), first_trial=128,
                 batch=len(rows))
    check(res, arrays(ref), f"given n={n} m={m}")
    # a loyal commander and |F| <= m (all three shapes have n > 3m): every loyal
    # lieutenant decides the order, in phase 1
    assert n > 3 * m
    lts = (1 << (2 * (n - 1))) - 1
    seen = 0
    for i, (f_, o_) in enumerate(rows):
        f_ &= full
        if not f_ & 1 and bin(f_).count("1") <= m:
            loyal = sum(3 << (2 * (r - 1)) for r in range(1, n) if not (f_ >> r) & 1)
            want = (0x5555555555555555 if o_ == 1 else 0) & lts
            assert int(res.decisions[i]) & loyal == want & loyal, (i, f_, o_)
            assert int(res.decided[i]) == 1, (i, f_, o_)
            seen += 1
    assert seen >= 24


def test_sharding_and_device_accumulation(engine):
    import torch
    from ba_amd import lib as L
    kw = dict(seed=SEEDS[1], faulty_mode=L.FAULTY_RANDOM, f=10, order_mode=L.ORDER_RANDOM)
    for policy, coin in zip(POLICIES, COINS):
        whole = engine.run_rand(10, 3, 256, 3, policy, coin, want_decided=True, **kw)
        a = engine.run_rand(10, 3, 128, 3, policy, coin, want_decided=True, **kw)
        b = engine.run_rand(10, 3, 128, 3, policy, coin, first_trial=128, want_decided=True, **kw)
        same(np.concatenate([a.decisions, b.decisions]), whole.decisions, "decisions")
        same(np.concatenate([a.outcome, b.outcome]), whole.outcome, "outcome")
        same(np.concatenate([a.decided, b.decided]), whole.decided, "decided")
        assert {k: a.counters[k] + b.counters[k] for k in a.counters} == whole.counters
        check(whole, model(10, 3, 3, policy, coin, 256, SEEDS[1], O.FAULTY_RANDOM, 10, O.ORDER_RANDOM),
              "whole")
        # the device entry accumulates into d_counters across calls
        cnt = torch.zeros(16, dtype=torch.int64, device="cuda")
        s = torch.cuda.current_stream().cuda_stream
        for first in (0, 128):
            engine.run_rand_device(L.make_params(10, 3, first_trial=first, **kw), 128, 3, policy, coin,
                                   d_counters=cnt.data_ptr(), stream=s)
        torch.cuda.synchronize()
        got = dict(zip(L.COUNTER_NAMES, cnt.cpu().tolist()))
        assert got == whole.counters
        assert cnt.cpu().tolist()[12:] == [0, 0, 0, 0]


SINK_B = 64 * 68 + 37  # 69 words: 18 four-wave blocks, 72 reporting waves > the sink's 64 replicas


@pytest.mark.parametrize("policy,coin", [(RM.KING_COIN, RM.RAND_COMMON), (RM.KING_SPLIT, RM.RAND_LOCAL)])
@pytest.mark.parametrize("n,m", [(10, 3), (4, 1)])
def test_sink_path_bit_exact(engine, n, m, policy, coin):
    """A launch of more than 64 reporting waves adds its counters through the sink's
    replicas, where the smaller batches above add straight into the caller's: the
    whole batch against the model through the host entry, then as two device calls
    accumulating into one d_counters, then twice whole through the device entry."""
    import torch
    from ba_amd import lib as L
    words = (SINK_B + 63) // 64
    assert 4 * ((words + 3) // 4) > 64  # launch_rand: one unit per wave, four-wave blocks
    first = 64 * 9
    kw = dict(seed=SEEDS[0], faulty_mode=L.FAULTY_RANDOM, f=n, order_mode=L.ORDER_RANDOM)
    ref = model(n, m, 2, policy, coin, SINK_B, SEEDS[0], O.FAULTY_RANDOM, n, O.ORDER_RANDOM, first)
    check(engine.run_rand(n, m, SINK_B, 2, policy, coin, first_trial=first, want_decided=True, **kw), ref,
          f"host n={n} m={m} policy={policy}")
    s = torch.cuda.current_stream().cuda_stream
    half = 64 * 34
    for what, calls, times in (("two halves", ((0, half), (half, SINK_B - half)), 1),
                               ("whole twice", ((0, SINK_B), (0, SINK_B)), 2)):
        dec = torch.full((SINK_B,), -1, dtype=torch.int64, device="cuda")
        out = torch.full((SINK_B,), 253, dtype=torch.uint8, device="cuda")
        dcd = torch.full((SINK_B,), 253, dtype=torch.uint8, device="cuda")
        cnt = torch.zeros(16, dtype=torch.int64, device="cuda")
        for t0, count in calls:
            engine.run_rand_device(L.make_params(n, m, first_trial=first + t0, **kw), count, 2, policy, coin,
                                   d_decisions=dec[t0:].data_ptr(), d_outcome=out[t0:].data_ptr(),
                                   d_decided=dcd[t0:].data_ptr(), d_counters=cnt.data_ptr(), stream=s)
        torch.cuda.synchronize()
        same(dec.cpu().numpy().view(np.uint64), ref[0], f"{what} decisions")
        same(out.cpu().numpy(), ref[1], f"{what} outcome")
        same(dcd.cpu().numpy(), ref[2], f"{what} decided")
        got = cnt.cpu().tolist()
        assert dict(zip(L.COUNTER_NAMES, got)) == {k: times * v for k, v in ref[3].items()}, what
        assert got[12:] == [0, 0, 0, 0]


def test_host_entry_chunks(engine, monkeypatch):
    """The host entry's chunk loop (forced to 64): same bits as one chunk."""
    from ba_amd import lib as L
    kw = dict(seed=SEEDS[0], faulty_mode=L.FAULTY_RANDOM, f=10, order_mode=L.ORDER_RANDOM)
    rng = np.random.default_rng(1)
    fm = rng.integers(0, 1 << 10, B, dtype=np.uint64).astype(np.uint32)
    oc = rng.choice([0, 1, 2], B).astype(np.uint8)
    C, S, LO, CO = RM.KING_COIN, RM.KING_SPLIT, RM.RAND_LOCAL, RM.RAND_COMMON
    one = engine.run_rand(10, 3, B, 3, C, CO, want_decided=True, **kw)
    one_g = engine.run_rand(10, 3, B, 3, S, LO, seed=3, faulty=fm, order=oc, want_decided=True)
    monkeypatch.setenv("BA_RAND_HOST_CHUNK", "64")
    for ref, res in ((one, engine.run_rand(10, 3, B, 3, C, CO, want_decided=True, **kw)),
                     (one_g, engine.run_rand(10, 3, B, 3, S, LO, seed=3, faulty=fm, order=oc,
                                             want_decided=True))):
        same(res.decisions, ref.decisions, "decisions")
        same(res.outcome, ref.outcome, "outcome")
        same(res.decided, ref.decided, "decided")
        assert res.counters == ref.counters
    check(one, model(10, 3, 3, C, CO, B, SEEDS[0], O.FAULTY_RANDOM, 10, O.ORDER_RANDOM), "one chunk")
    check(one_g, arrays(RM.run(10, 3, 3, S, LO, seed=3, faulty=fm.tolist(), order=oc.tolist(), batch=B)),
          "one chunk, given")


@pytest.mark.parametrize("coin", COINS)
def test_staged_inputs_equal_in_kernel_draws_and_optional_outputs(engine, coin):
    """ba_gen_inputs_device + GIVEN == drawing in the kernel; the decisions, outcome
    and decided pointers are each optional, in every combination, and an absent
    buffer is not touched."""
    import torch
    from ba_amd import lib as L
    n, m, R = 10, 3, 3
    kw = dict(seed=SEEDS[0], faulty_mode=L.FAULTY_RANDOM, f=n, order_mode=L.ORDER_RANDOM)
    ref = model(n, m, R, RM.KING_COIN, coin, B, SEEDS[0], O.FAULTY_RANDOM, n, O.ORDER_RANDOM)
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
            out = torch.full((B,), 253, dtype=torch.uint8, device="cuda")
            dcd = torch.full((B,), 253, dtype=torch.uint8, device="cuda")
            cnt = torch.zeros(16, dtype=torch.int64, device="cuda")
            engine.run_rand_device(p, B, R, RM.KING_COIN, coin, d_decisions=dec.data_ptr() if wd else 0,
                                   d_outcome=out.data_ptr() if wo else 0,
                                   d_decided=dcd.data_ptr() if ws else 0, d_counters=cnt.data_ptr(),
                                   stream=s, **ins)
            torch.cuda.synchronize()
            what = f"given={p is given} dec={wd} out={wo} decided={ws}"
            same(dec.cpu().numpy().view(np.uint64), ref[0] if wd else np.full(B, 2**64 - 1, np.uint64),
                 what + " decisions")
            same(out.cpu().numpy(), ref[1] if wo else np.full(B, 253, np.uint8), what + " outcome")
            same(dcd.cpu().numpy(), ref[2] if ws else np.full(B, 253, np.uint8), what + " decided")
            assert dict(zip(L.COUNTER_NAMES, cnt.cpu().tolist())) == ref[3], what


@pytest.mark.parametrize("n,m,policy,coin", [(10, 3, RM.KING_COIN, RM.RAND_COMMON),
                                             (4, 1, RM.KING_SPLIT, RM.RAND_LOCAL)])
def test_graph_capture_and_replay(n, m, policy, coin):
    """The device entry captured after the identical eager call and replayed three
    times, with d_counters left alone and zeroed in the graph; between replays 2 and 3
    the ctx makes an eager OM call (the frame of tests/test_gpu_ctx_state.py)."""
    import torch
    import test_gpu_ctx_state as G
    from ba_amd import lib as L
    assert G.wave_units(G.B69) > 64
    R, kw = 3, G.model_kw(n)
    dec, out, dcd, cnt = RM.run(n, m, R, policy, coin, batch=G.B69, **kw)
    want = {"decisions": np.array(dec, np.uint64), "outcome": np.array(out, np.uint8),
            "decided": np.array(dcd, np.uint8)}

    def make():
        outs = G._bufs(G.B69, decided=torch.uint8)
        c = G.Call(f"rand({n},{m}) policy={policy} coin={coin}", G.B69, outs, want, cnt)
        c.issue = lambda e, s: e.run_rand_device(
            L.make_params(n, m, **kw), G.B69, R, policy, coin, d_decisions=outs["decisions"].data_ptr(),
            d_outcome=outs["outcome"].data_ptr(), d_decided=outs["decided"].data_ptr(),
            d_counters=c.cnt.data_ptr(), stream=s)
        return c

    G.graph_rounds(make, between=lambda: G.om_call(10, 3, 777))


@pytest.mark.parametrize("n,m", [(7, 2), (10, 3)])
def test_theory_consequences(engine, n, m):
    """Consequences of §13's arguments on the GPU results, 4,096 trials, R = 6, both
    policies and coins: no trial in bound is unsafe; in bound with a loyal commander
    everyone decides in phase 1 and IC2 holds; without a traitor everyone decides in
    phase 1; an in-bound trial breaks IC1 or IC2 only while somebody is undecided."""
    from ba_amd import lib as L
    T, R = 4096, 6
    for policy, coin in itertools.product(POLICIES, COINS):
        res = engine.run_rand(n, m, T, R, policy, coin, seed=2024, faulty_mode=L.FAULTY_RANDOM, f=n,
                              order_mode=L.ORDER_RANDOM, want_decided=True)
        out, dcd = res.outcome.astype(np.uint32), res.decided
        agree, appl, valid, inb = ((out >> b) & 1 == 1 for b in (2, 3, 4, 5))
        assert res.counters["trials"] == T and 0 < inb.sum() < T
        assert inb.sum() == res.counters["in_bound"]
        assert not np.any(dcd[inb] == RM.UNSAFE)
        loyal_cmd = inb & appl
        assert loyal_cmd.any()
        assert np.all(dcd[loyal_cmd] == 1) and np.all(valid[loyal_cmd]) and np.all(agree[loyal_cmd])
        viol = inb & (~agree | (appl & ~valid))
        assert viol.sum() == res.counters["bound_violations"]
        assert viol.sum() <= (inb & (dcd == RM.UNDECIDED)).sum()
        assert not np.any(viol & (dcd != RM.UNDECIDED))
        none = engine.run_rand(n, m, T, R, policy, coin, seed=2024, faulty_mode=L.FAULTY_EXACT, f=0,
                               order_mode=L.ORDER_RANDOM, want_decided=True)
        assert np.all(none.decided == 1)
        assert none.counters["agreement"] == T and none.counters["validity"] == T
        assert none.counters["bound_violations"] == 0


def test_errors(engine):
    from ba_amd import lib as L
    kw = dict(faulty_mode=L.FAULTY_EXACT, f=0, order_mode=L.ORDER_CONST)

    def code(**over):
        a = dict(n=4, m=1, batch=64, phases=2, policy=RM.KING_COIN, coin=RM.RAND_COMMON)
        a.update(kw)
        a.update(over)
        with pytest.raises(L.BAError) as e:
            engine.run_rand(a.pop("n"), a.pop("m"), a.pop("batch"), a.pop("phases"), a.pop("policy"),
                            a.pop("coin"), **a)
        return e.value.code

    assert code(lie_mode=L.LIE_TABLE) == L.ENOTSUP
    assert code(n=0) == L.EINVAL
    assert code(n=33) == L.EINVAL
    assert code(n=32, m=11) == L.EINVAL
    assert engine.run_rand(32, 10, 64, 1, **kw).counters["trials"] == 64  # m = 10 is accepted
    assert code(policy=2) == L.EINVAL
    assert code(coin=2) == L.EINVAL
    assert code(phases=0) == L.EINVAL
    assert code(phases=65) == L.EINVAL
    assert engine.run_rand(4, 1, 64, 64, **kw).counters["trials"] == 64  # R = 64 is accepted
    assert code(first_trial=32) == L.EINVAL
    assert code(faulty_mode=L.FAULTY_GIVEN) == L.EINVAL  # no faulty_mask
    assert code(order_mode=L.ORDER_GIVEN) == L.EINVAL    # no order
    for eng in (L.ENGINE_FUSED, L.ENGINE_LEVELS):
        assert code(engine=eng) == L.EINVAL
        assert b"engine" in engine.lib.ba_last_error()
    # the device entry validates alike, and needs d_counters
    with pytest.raises(L.BAError) as e:
        engine.run_rand_device(L.make_params(4, 1, **kw), 64, 65)
    assert e.value.code == L.EINVAL
    with pytest.raises(L.BAError) as e:
        engine.run_rand_device(L.make_params(4, 1, **kw), 64, 2)
    assert e.value.code == L.EINVAL and "d_counters" in str(e.value)
    # the trial index may not wrap: the last trial is at most 2^64 - 1
    with pytest.raises(L.BAError) as e:
        engine.run_rand(4, 1, 65, 2, first_trial=2**64 - 64, **kw)
    assert e.value.code == L.EINVAL and "first_trial" in str(e.value)
    kr = dict(seed=5, faulty_mode=L.FAULTY_RANDOM, f=4, order_mode=L.ORDER_RANDOM)
    top = engine.run_rand(4, 1, 64, 2, first_trial=2**64 - 64, want_decided=True, **kr)  # ends at 2^64
    check(top, arrays(RM.run(4, 1, 2, first_trial=2**64 - 64, batch=64, **kr)), "top")
    # batch = 0: BA_OK with zero counters
    res = engine.run_rand(4, 1, 0, 2, **kw)
    assert all(v == 0 for v in res.counters.values())
    # NULL params are an error, not a crash
    cnt = L.Counters()
    assert engine.lib.ba_rand_run_trials(engine.handle, None, 0, 1, 2, 64, None, None, None, None, None,
                                         ctypes.byref(cnt)) == L.EINVAL
    # the ctx still works
    assert engine.run_rand(4, 1, 64, 2, **kw).counters["trials"] == 64
