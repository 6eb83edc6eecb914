"""GPU tests of SM(m), signed messages (docs/SEMANTICS.md §6): k_sm through the C
ABI against the chain-form reference model (tests/sm_model.py).  Every
comparison is exact: decisions, outcome bytes, V sets and all 12 run counters."""
import functools
import itertools

import numpy as np
import pytest

import ba_oracle as O
import sm_model as S

pytestmark = pytest.mark.gpu

# (9,3): 56 pairs < 64 lanes; (10,3): 72 and (12,2): 110 pairs, a second pass over
# the lanes; (32,8): 930 pairs, groups of four passes; (4,5): m > me; n <= 2: no relay
SHAPES = [(1, 0), (2, 1), (3, 1), (4, 0), (4, 1), (4, 5), (5, 2), (9, 3), (10, 3), (12, 2), (32, 8)]
SEEDS = [0xBA5EED, 0x5157ED0123456789]
B = 229  # three full words and a partial one


@functools.lru_cache(maxsize=None)
def model(n, m, batch, seed, faulty_mode, f, order_mode, first_trial=0):
    """Reference results of a run that draws its own inputs (computed once, shared)."""
    dec, out, vs, cnt = S.run(n, m, seed=seed, faulty_mode=faulty_mode, f=f, order_mode=order_mode,
                              first_trial=first_trial, batch=batch)
    return (np.array(dec, np.uint64), np.array(out, np.uint8), np.array(vs, np.uint64), cnt)


def same(a, b, what):
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape, f"{what}: shape {a.shape} != {b.shape}"
    if not np.array_equal(a, b):
        idx = np.nonzero(a != b)[0]
        raise AssertionError(f"{what}: {len(idx)} mismatches, first at {idx[:5].tolist()}: "
                             f"got {a[idx[:5]].tolist()} want {b[idx[:5]].tolist()}")


def check(res, ref, what):
    dec, out, vs, cnt = ref
    same(res.decisions, dec, f"{what} decisions")
    same(res.outcome, out, f"{what} outcome")
    same(res.vsets, vs, f"{what} vsets")
    assert len(cnt) == 12
    assert {k: res.counters[k] for k in cnt} == cnt, what


@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("n,m", SHAPES)
def test_shapes_bit_exact(engine, n, m, seed):
    from ba_amd import lib as L
    res = engine.run_sm(n, m, B, seed=seed, faulty_mode=L.FAULTY_RANDOM, f=n,
                        order_mode=L.ORDER_RANDOM, want_vsets=True)
    check(res, model(n, m, B, seed, O.FAULTY_RANDOM, n, O.ORDER_RANDOM), f"n={n} m={m}")
    assert res.counters["undefined_decisions"] == 0


@pytest.mark.parametrize("first", [0, 64 * 5, 1 << 38])
def test_first_trial(engine, first):
    from ba_amd import lib as L
    res = engine.run_sm(10, 3, B, seed=SEEDS[0], faulty_mode=L.FAULTY_RANDOM, f=10,
                        order_mode=L.ORDER_RANDOM, first_trial=first, want_vsets=True)
    check(res, model(10, 3, B, SEEDS[0], O.FAULTY_RANDOM, 10, O.ORDER_RANDOM, first), f"first={first}")


@pytest.mark.parametrize("n,m", [(4, 1), (10, 3), (32, 2)])
def test_given_inputs(engine, n, m):
    """No traitor, every general faulty, a faulty commander only, mask bits at and
    above n (ignored), and every order code, BA_OTHER included."""
    full = (1 << n) - 1
    high = (0xFFFFFFFF & ~full) if n < 32 else 0
    masks = [0, full, 1, high, high | 1, high | full, 0b110 & full, full & ~1]
    rows = [(fm, oc) for fm in masks for oc in (0, 1, 2)]
    rows = rows * 4  # 96 trials: two words, the coins differ per trial
    fm = np.array([r[0] for r in rows], np.uint32)
    oc = np.array([r[1] for r in rows], np.uint8)
    res = engine.run_sm(n, m, len(rows), seed=99, faulty=fm, order=oc, first_trial=128, want_vsets=True)
    dec, out, vs, cnt = S.run(n, m, seed=99, faulty=fm.tolist(), order=oc.tolist(), first_trial=128,
                              batch=len(rows))
    check(res, (np.array(dec, np.uint64), np.array(out, np.uint8), np.array(vs, np.uint64), cnt),
          f"given n={n} m={m}")
    # a loyal commander: every lieutenant's V is exactly {order}
    want = {0: 0xAAAAAAAAAAAAAAAA, 1: 0x5555555555555555, 2: 0xAAAAAAAAAAAAAAAA}
    lts = (1 << (2 * (n - 1))) - 1
    for i, (f_, o_) in enumerate(rows):
        if not f_ & 1:
            assert int(res.vsets[i]) == want[o_] & lts, (i, f_, o_)


def test_loyal_commander_vsets_random_sets(engine):
    from ba_amd import lib as L
    n, m = 10, 3
    res = engine.run_sm(n, m, 4096, seed=5, faulty_mode=L.FAULTY_RANDOM, f=n, order_mode=L.ORDER_RANDOM,
                        want_vsets=True)
    appl = (res.outcome >> 3) & 1 == 1
    assert appl.any() and not appl.all()
    vs = res.vsets[appl]
    lts = np.uint64((1 << (2 * (n - 1))) - 1)
    assert np.all((vs == np.uint64(0x5555555555555555) & lts) | (vs == np.uint64(0xAAAAAAAAAAAAAAAA) & lts))
    # the decision follows: V = {attack} -> attack codes everywhere, else retreat
    same(res.decisions[appl], vs & np.uint64(0x5555555555555555), "decisions of loyal-commander trials")


SINK_B = 64 * 68 + 37  # 69 words: 18 four-wave blocks, 72 reporting waves > the sink's 64 replicas


@pytest.mark.parametrize("n,m", [(10, 3), (4, 1)])
def test_sink_path_bit_exact(engine, n, m):
    """A launch of more than 64 reporting waves adds its counters through the sink's
    replicas (sink_counters, ba_device.hpp), where the smaller batches above add
    straight into the caller's: the whole batch against the model through the host
    entry, then as two device calls accumulating into one d_counters, then twice
    whole through the device entry (the first launch must leave the replicas zero)."""
    import torch
    from ba_amd import lib as L
    words = (SINK_B + 63) // 64
    assert 4 * ((words + 3) // 4) > 64  # launch_sm: one unit per wave, four-wave blocks
    first = 64 * 9
    kw = dict(seed=SEEDS[0], faulty_mode=L.FAULTY_RANDOM, f=n, order_mode=L.ORDER_RANDOM)
    ref = model(n, m, SINK_B, SEEDS[0], O.FAULTY_RANDOM, n, O.ORDER_RANDOM, first)
    check(engine.run_sm(n, m, SINK_B, first_trial=first, want_vsets=True, **kw), ref, f"host n={n} m={m}")
    s = torch.cuda.current_stream().cuda_stream
    half = 64 * 34
    for what, calls, times in (("two halves", ((0, half), (half, SINK_B - half)), 1),
                               ("whole twice", ((0, SINK_B), (0, SINK_B)), 2)):
        dec = torch.full((SINK_B,), -1, dtype=torch.int64, device="cuda")
        out = torch.full((SINK_B,), 254, dtype=torch.uint8, device="cuda")
        vs = torch.full((SINK_B,), -1, dtype=torch.int64, device="cuda")
        cnt = torch.zeros(16, dtype=torch.int64, device="cuda")
        for t0, count in calls:
            engine.run_sm_device(L.make_params(n, m, first_trial=first + t0, **kw), count,
                                 d_decisions=dec[t0:].data_ptr(), d_outcome=out[t0:].data_ptr(),
                                 d_vsets=vs[t0:].data_ptr(), d_counters=cnt.data_ptr(), stream=s)
        torch.cuda.synchronize()
        same(dec.cpu().numpy().view(np.uint64), ref[0], f"{what} decisions")
        same(out.cpu().numpy(), ref[1], f"{what} outcome")
        same(vs.cpu().numpy().view(np.uint64), ref[2], f"{what} vsets")
        got = cnt.cpu().tolist()
        assert dict(zip(L.COUNTER_NAMES, got)) == {k: times * v for k, v in ref[3].items()}, what
        assert got[12:] == [0, 0, 0, 0]


def test_sharding_and_device_accumulation(engine):
    import torch
    from ba_amd import lib as L
    kw = dict(seed=SEEDS[1], faulty_mode=L.FAULTY_RANDOM, f=10, order_mode=L.ORDER_RANDOM)
    whole = engine.run_sm(10, 3, 256, want_vsets=True, **kw)
    a = engine.run_sm(10, 3, 128, want_vsets=True, **kw)
    b = engine.run_sm(10, 3, 128, first_trial=128, want_vsets=True, **kw)
    same(np.concatenate([a.decisions, b.decisions]), whole.decisions, "decisions")
    same(np.concatenate([a.outcome, b.outcome]), whole.outcome, "outcome")
    same(np.concatenate([a.vsets, b.vsets]), whole.vsets, "vsets")
    assert {k: a.counters[k] + b.counters[k] for k in a.counters} == whole.counters
    check(whole, model(10, 3, 256, SEEDS[1], O.FAULTY_RANDOM, 10, O.ORDER_RANDOM), "whole")
    # the device entry accumulates into d_counters across calls
    cnt = torch.zeros(16, dtype=torch.int64, device="cuda")
    s = torch.cuda.current_stream().cuda_stream
    for first in (0, 128):
        engine.run_sm_device(L.make_params(10, 3, first_trial=first, **kw), 128,
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
    one = engine.run_sm(10, 3, B, want_vsets=True, **kw)
    one_g = engine.run_sm(10, 3, B, seed=3, faulty=fm, order=oc, want_vsets=True)
    monkeypatch.setenv("BA_SM_HOST_CHUNK", "64")
    for ref, res in ((one, engine.run_sm(10, 3, B, want_vsets=True, **kw)),
                     (one_g, engine.run_sm(10, 3, B, seed=3, faulty=fm, order=oc, want_vsets=True))):
        same(res.decisions, ref.decisions, "decisions")
        same(res.outcome, ref.outcome, "outcome")
        same(res.vsets, ref.vsets, "vsets")
        assert res.counters == ref.counters
    check(one, model(10, 3, B, SEEDS[0], O.FAULTY_RANDOM, 10, O.ORDER_RANDOM), "one chunk")


def test_host_entry_vsets_without_decisions(engine, monkeypatch):
    """The extra plane alone through the chunked host entry: the V sets ride behind the
    decisions in one staging buffer and are asked for without them (64-trial chunks, a
    partial last word)."""
    from ba_amd import lib as L
    n, m, b = 4, 1, 130
    monkeypatch.setenv("BA_SM_HOST_CHUNK", "64")
    res = engine.run_sm(n, m, b, seed=SEEDS[0], faulty_mode=L.FAULTY_RANDOM, f=n,
                        order_mode=L.ORDER_RANDOM, want_decisions=False, want_outcome=False,
                        want_vsets=True)
    ref = model(n, m, b, SEEDS[0], O.FAULTY_RANDOM, n, O.ORDER_RANDOM)
    assert res.decisions is None and res.outcome is None
    same(res.vsets, ref[2], "vsets")
    assert {k: res.counters[k] for k in ref[3]} == ref[3]


def test_staged_inputs_equal_in_kernel_draws_and_optional_outputs(engine):
    """ba_gen_inputs_device + GIVEN == drawing in the kernel; the decisions, outcome
    and vsets pointers are each optional, in every combination."""
    import torch
    from ba_amd import lib as L
    n, m = 10, 3
    kw = dict(seed=SEEDS[0], faulty_mode=L.FAULTY_RANDOM, f=n, order_mode=L.ORDER_RANDOM)
    ref = model(n, m, B, SEEDS[0], O.FAULTY_RANDOM, n, O.ORDER_RANDOM)
    s = torch.cuda.current_stream().cuda_stream
    fm = torch.zeros(B, dtype=torch.int32, device="cuda")
    oc = torch.zeros(B, dtype=torch.uint8, device="cuda")
    engine.gen_inputs_device(L.make_params(n, m, **kw), B, d_faulty=fm.data_ptr(), d_order=oc.data_ptr(),
                             stream=s)
    given = L.make_params(n, m, seed=SEEDS[0])
    drawn = L.make_params(n, m, **kw)
    for p, ins in ((given, dict(d_faulty=fm.data_ptr(), d_order=oc.data_ptr())), (drawn, {})):
        for wd, wo, wv in itertools.product((False, True), repeat=3):
            dec = torch.full((B,), -1, dtype=torch.int64, device="cuda")
            out = torch.full((B,), 255, dtype=torch.uint8, device="cuda")
            vs = torch.full((B,), -1, dtype=torch.int64, device="cuda")
            cnt = torch.zeros(16, dtype=torch.int64, device="cuda")
            engine.run_sm_device(p, B, d_decisions=dec.data_ptr() if wd else 0,
                                 d_outcome=out.data_ptr() if wo else 0,
                                 d_vsets=vs.data_ptr() if wv else 0, d_counters=cnt.data_ptr(),
                                 stream=s, **ins)
            torch.cuda.synchronize()
            what = f"given={p is given} dec={wd} out={wo} vsets={wv}"
            same(dec.cpu().numpy().view(np.uint64), ref[0] if wd else np.full(B, 2**64 - 1, np.uint64),
                 what + " decisions")
            same(out.cpu().numpy(), ref[1] if wo else np.full(B, 255, np.uint8), what + " outcome")
            same(vs.cpu().numpy().view(np.uint64), ref[2] if wv else np.full(B, 2**64 - 1, np.uint64),
                 what + " vsets")
            assert dict(zip(L.COUNTER_NAMES, cnt.cpu().tolist())) == ref[3], what


def test_theory_counters(engine):
    """Lamport's theorem on counters alone, 65,536 trials each: f <= m never breaks
    IC1 or IC2 whatever n; f > m can."""
    from ba_amd import lib as L
    T = 65536
    kw = dict(seed=2024, order_mode=L.ORDER_RANDOM, want_decisions=False, want_outcome=False)
    for n, m, mode, f in ((4, 2, L.FAULTY_EXACT, 2), (10, 3, L.FAULTY_RANDOM, 3)):
        c = engine.run_sm(n, m, T, faulty_mode=mode, f=f, **kw).counters
        assert c["trials"] == T and c["in_bound"] == T
        assert c["bound_violations"] == 0 and c["agreement"] == T
        assert c["validity"] == c["validity_applicable"]
        assert c["undefined_decisions"] == 0
    c = engine.run_sm(4, 1, T, faulty_mode=L.FAULTY_EXACT, f=2, **kw).counters
    assert c["trials"] == T and c["in_bound"] == 0 and c["bound_violations"] == 0
    assert c["agreement"] < T
    assert c["undefined_decisions"] == 0 and c["faulty_total"] == 2 * T


def test_errors(engine):
    from ba_amd import lib as L
    kw = dict(faulty_mode=L.FAULTY_EXACT, f=0, order_mode=L.ORDER_CONST)

    def code(**over):
        a = dict(n=4, m=1, batch=64)
        a.update(kw)
        a.update(over)
        with pytest.raises(L.BAError) as e:
            engine.run_sm(a.pop("n"), a.pop("m"), a.pop("batch"), **a)
        return e.value.code

    assert code(lie_mode=L.LIE_TABLE) == L.ENOTSUP
    assert code(n=0) == L.EINVAL
    assert code(n=33) == L.EINVAL
    assert code(m=9) == L.EINVAL
    assert code(first_trial=32) == L.EINVAL
    assert code(faulty_mode=L.FAULTY_GIVEN) == L.EINVAL  # no faulty_mask
    assert code(order_mode=L.ORDER_GIVEN) == L.EINVAL    # no order
    for eng in (L.ENGINE_FUSED, L.ENGINE_LEVELS):
        p = L.make_params(4, 1, engine=eng, **kw)
        cnt = L.Counters()
        import ctypes
        rc = engine.lib.ba_sm_run_trials(engine.handle, ctypes.byref(p), 64, None, None, None, None,
                                         None, ctypes.byref(cnt))
        assert rc == L.EINVAL and b"engine" in engine.lib.ba_last_error()
    # the trial index may not wrap: the last trial is at most 2^64 - 1
    with pytest.raises(L.BAError) as e:
        engine.run_sm(4, 1, 65, first_trial=2**64 - 64, **kw)
    assert e.value.code == L.EINVAL and "first_trial" in str(e.value)
    top = engine.run_sm(4, 1, 64, first_trial=2**64 - 64, want_vsets=True, **kw)  # ends at 2^64: valid
    dec, out, vs, cnt = S.run(4, 1, first_trial=2**64 - 64, batch=64, **kw)
    check(top, (np.array(dec, np.uint64), np.array(out, np.uint8), np.array(vs, np.uint64), cnt), "top")
    # batch = 0: BA_OK with zero counters
    res = engine.run_sm(4, 1, 0, **kw)
    assert all(v == 0 for v in res.counters.values())
    # the ctx still works
    assert engine.run_sm(4, 1, 64, **kw).counters["trials"] == 64


def test_bench_size_equals_sum_of_sixteen(engine):
    """1,048,576 trials at (10, 3) in one call == sixteen 65,536-trial calls:
    the persistent word loop and the counter sink at bench size."""
    from ba_amd import lib as L
    kw = dict(seed=0xBA5EED, faulty_mode=L.FAULTY_RANDOM, f=3, order_mode=L.ORDER_RANDOM,
              want_decisions=False, want_outcome=False)
    T, K = 1 << 20, 16
    whole = engine.run_sm(10, 3, T, **kw).counters
    tot = dict.fromkeys(whole, 0)
    for i in range(K):
        c = engine.run_sm(10, 3, T // K, first_trial=i * (T // K), **kw).counters
        for k in tot:
            tot[k] += c[k]
    assert whole == tot
    assert whole["trials"] == T and whole["bound_violations"] == 0
