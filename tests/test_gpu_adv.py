"""GPU tests of OM(m) under scripted traitor policies (docs/SEMANTICS.md §7): k_adv
through the C ABI against the level-array reference model (tests/adv_model.py).
Every comparison is exact: decisions, outcome bytes and all 12 run counters."""
import ctypes
import functools
import itertools

import numpy as np
import pytest

import adv_model as A
import ba_oracle as O

pytestmark = pytest.mark.gpu

# (n, m, batch).  229 = three full words and a partial one.  n <= 2: no relay;
# (4,0), (4,5), (7,5): m = 0 and m > me; (8,4), (10,3): several words per wave;
# (9,8): depth 7; (32,1), (32,2): 31 receivers per word, the widest counters
SHAPES = [(1, 0, 229), (2, 1, 229), (3, 1, 229), (4, 0, 229), (4, 1, 229), (4, 5, 229),
          (5, 2, 229), (7, 5, 229), (8, 4, 229), (10, 3, 229), (9, 8, 70), (32, 1, 70), (32, 2, 70)]
SEEDS = [0xBA5EED, 0x5157ED0123456789]
B = 229


@functools.lru_cache(maxsize=None)
def model(n, m, policy, batch, seed, first_trial=0):
    """Reference results of a run that draws its own inputs (computed once, shared)."""
    dec, out, cnt = A.run(n, m, policy, seed=seed, faulty_mode=O.FAULTY_RANDOM, f=n,
                          order_mode=O.ORDER_RANDOM, first_trial=first_trial, batch=batch)
    return np.array(dec, np.uint64), np.array(out, np.uint8), cnt


def given_model(n, m, policy, fm, oc, **kw):
    dec, out, cnt = A.run(n, m, policy, faulty=[int(x) for x in fm], order=[int(x) for x in oc],
                          batch=len(fm), **kw)
    return np.array(dec, np.uint64), np.array(out, np.uint8), cnt


def same(a, b, what):
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape, f"{what}: shape {a.shape} != {b.shape}"
    if not np.array_equal(a, b):
        idx = np.nonzero(a != b)[0]
        raise AssertionError(f"{what}: {len(idx)} mismatches, first at {idx[:5].tolist()}: "
                             f"got {a[idx[:5]].tolist()} want {b[idx[:5]].tolist()}")


def check(res, ref, what):
    dec, out, cnt = ref
    same(res.decisions, dec, f"{what} decisions")
    same(res.outcome, out, f"{what} outcome")
    assert len(cnt) == 12
    assert {k: res.counters[k] for k in cnt} == cnt, what


def drawn(L):
    return dict(faulty_mode=L.FAULTY_RANDOM, order_mode=L.ORDER_RANDOM)


@pytest.mark.parametrize("policy", A.POLICIES)
@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("n,m,batch", SHAPES)
def test_shapes_bit_exact(engine, n, m, batch, seed, policy):
    from ba_amd import lib as L
    res = engine.run_adv(n, m, batch, policy, seed=seed, f=n, **drawn(L))
    check(res, model(n, m, policy, batch, seed), f"n={n} m={m} policy={policy}")


def adv_units(n, batch):
    """Reporting waves of launch_adv (ba_adv.hip): four per block, a block per
    wpb = min(32, 256 // (n - 1)) trial words (below the per-CU block cap)."""
    wpb = min(32, 256 // (n - 1))
    words = (batch + 63) // 64
    return 4 * ((words + wpb - 1) // wpb)


@pytest.mark.parametrize("policy", A.POLICIES)
@pytest.mark.parametrize("n,m", [(10, 3), (4, 1)])
def test_sink_path_bit_exact(engine, n, m, policy):
    """A launch of more than 64 reporting waves adds its counters through the sink's
    replicas (sink_counters, ba_device.hpp), where the smaller batches above add
    straight into the caller's.  A k_adv block takes wpb words, so that is 16 wpb + 1
    words: 17 blocks, 68 waves.  The whole batch against the model through the host
    entry, then as two device calls accumulating into one d_counters, then twice whole
    through the device entry (the first launch must leave the replicas zero)."""
    import torch
    from ba_amd import lib as L
    wpb = min(32, 256 // (n - 1))
    Bs = 64 * 16 * wpb + 37
    assert adv_units(n, Bs) == 68 and adv_units(n, 64 * 16 * wpb) == 64
    first = 64 * 9
    kw = dict(seed=SEEDS[0], f=n, **drawn(L))
    ref = model(n, m, policy, Bs, SEEDS[0], first)
    check(engine.run_adv(n, m, Bs, policy, first_trial=first, **kw), ref, f"host n={n} m={m} policy={policy}")
    s = torch.cuda.current_stream().cuda_stream
    half = 64 * 8 * wpb
    for what, calls, times in (("two halves", ((0, half), (half, Bs - half)), 1),
                               ("whole twice", ((0, Bs), (0, Bs)), 2)):
        dec = torch.full((Bs,), -1, dtype=torch.int64, device="cuda")
        out = torch.full((Bs,), 254, dtype=torch.uint8, device="cuda")
        cnt = torch.zeros(16, dtype=torch.int64, device="cuda")
        for t0, count in calls:
            engine.run_adv_device(L.make_params(n, m, first_trial=first + t0, **kw), count, policy,
                                  d_decisions=dec[t0:].data_ptr(), d_outcome=out[t0:].data_ptr(),
                                  d_counters=cnt.data_ptr(), stream=s)
        torch.cuda.synchronize()
        same(dec.cpu().numpy().view(np.uint64), ref[0], f"{what} decisions")
        same(out.cpu().numpy(), ref[1], f"{what} outcome")
        got = cnt.cpu().tolist()
        assert dict(zip(L.COUNTER_NAMES, got)) == {k: times * v for k, v in ref[2].items()}, what
        assert got[12:] == [0, 0, 0, 0]


@pytest.mark.parametrize("policy", A.POLICIES)
def test_depth_eight(engine, policy):
    """(10, 8): me = 8, 40,320 chains per receiver, on five given trials."""
    fm = np.array([0, 0b1111111111, 0b0000000110, 0b1010010011, 0b0101101100], np.uint32)
    oc = np.array([1, 0, 1, 2, 0], np.uint8)
    res = engine.run_adv(10, 8, 5, policy, faulty=fm, order=oc)
    check(res, given_model(10, 8, policy, fm, oc), f"depth 8 policy={policy}")


@pytest.mark.parametrize("policy", A.POLICIES)
@pytest.mark.parametrize("m", [1, 2])
def test_exhaustive_given_inputs(engine, m, policy):
    """Every faulty mask x every order code for n = 3..6 as one batch each, then the
    same rows with mask bits at and above n set (ignored)."""
    for n in (3, 4, 5, 6):
        rows = [(fm, oc) for fm in range(1 << n) for oc in (0, 1, 2)]
        high = 0xFFFFFFFF & ~((1 << n) - 1)
        fm = np.array([r[0] for r in rows] + [r[0] | high for r in rows], np.uint32)
        oc = np.array([r[1] for r in rows] * 2, np.uint8)
        res = engine.run_adv(n, m, len(fm), policy, faulty=fm, order=oc)
        ref = given_model(n, m, policy, fm, oc)
        check(res, ref, f"exhaustive n={n} m={m} policy={policy}")
        assert res.counters["bound_violations"] == 0
        same(res.decisions[len(rows):], res.decisions[:len(rows)], "high mask bits: decisions")
        same(res.outcome[len(rows):], res.outcome[:len(rows)], "high mask bits: outcome")
        if (n, m, policy) == (5, 1, A.ANTI):  # two traitors break OM(1) over 5 generals, always
            two = [i for i, r in enumerate(rows) if bin(r[0]).count("1") == 2 and r[1] != 2]
            assert len(two) == 20
            assert all(A.violated(int(res.outcome[i])) for i in two)


@pytest.mark.parametrize("policy", A.POLICIES)
@pytest.mark.parametrize("first", [0, 64 * 5, 1 << 38])
def test_first_trial(engine, first, policy):
    from ba_amd import lib as L
    res = engine.run_adv(10, 3, B, policy, seed=SEEDS[0], f=10, first_trial=first, **drawn(L))
    check(res, model(10, 3, policy, B, SEEDS[0], first), f"first={first}")


def test_given_inputs_do_not_depend_on_seed_or_first_trial(engine):
    rng = np.random.default_rng(7)
    fm = rng.integers(0, 1 << 10, B, dtype=np.uint64).astype(np.uint32)
    oc = rng.choice([0, 1, 2], B).astype(np.uint8)
    for policy in A.POLICIES:
        ref = engine.run_adv(10, 3, B, policy, faulty=fm, order=oc)
        check(ref, given_model(10, 3, policy, fm, oc), f"given policy={policy}")
        for seed, first in ((1, 0), (SEEDS[1], 64), (0, 1 << 38)):
            res = engine.run_adv(10, 3, B, policy, seed=seed, first_trial=first, faulty=fm, order=oc)
            same(res.decisions, ref.decisions, "decisions")
            same(res.outcome, ref.outcome, "outcome")
            assert res.counters == ref.counters


def test_staged_inputs_equal_in_kernel_draws_and_optional_outputs(engine):
    """ba_gen_inputs_device + GIVEN == drawing in the kernel; the decisions and outcome
    pointers are each optional, in every combination."""
    import torch
    from ba_amd import lib as L
    n, m, policy = 10, 3, A.ANTI
    kw = dict(seed=SEEDS[0], f=n, **drawn(L))
    ref = model(n, m, policy, B, SEEDS[0])
    s = torch.cuda.current_stream().cuda_stream
    fm = torch.zeros(B, dtype=torch.int32, device="cuda")
    oc = torch.zeros(B, dtype=torch.uint8, device="cuda")
    engine.gen_inputs_device(L.make_params(n, m, **kw), B, d_faulty=fm.data_ptr(), d_order=oc.data_ptr(),
                             stream=s)
    given = L.make_params(n, m, seed=SEEDS[0])
    for p, ins in ((given, dict(d_faulty=fm.data_ptr(), d_order=oc.data_ptr())),
                   (L.make_params(n, m, **kw), {})):
        for wd, wo in itertools.product((False, True), repeat=2):
            dec = torch.full((B,), -1, dtype=torch.int64, device="cuda")
            out = torch.full((B,), 255, dtype=torch.uint8, device="cuda")
            cnt = torch.zeros(16, dtype=torch.int64, device="cuda")
            engine.run_adv_device(p, B, policy, d_decisions=dec.data_ptr() if wd else 0,
                                  d_outcome=out.data_ptr() if wo else 0, d_counters=cnt.data_ptr(),
                                  stream=s, **ins)
            torch.cuda.synchronize()
            what = f"given={p is given} dec={wd} out={wo}"
            same(dec.cpu().numpy().view(np.uint64), ref[0] if wd else np.full(B, 2**64 - 1, np.uint64),
                 what + " decisions")
            same(out.cpu().numpy(), ref[1] if wo else np.full(B, 255, np.uint8), what + " outcome")
            assert dict(zip(L.COUNTER_NAMES, cnt.cpu().tolist())) == ref[2], what
    # the host entry: each output optional too
    for wd, wo in itertools.product((False, True), repeat=2):
        res = engine.run_adv(n, m, B, policy, want_decisions=wd, want_outcome=wo, **kw)
        assert (res.decisions is None) == (not wd) and (res.outcome is None) == (not wo)
        if wd:
            same(res.decisions, ref[0], "host decisions")
        if wo:
            same(res.outcome, ref[1], "host outcome")
        assert res.counters == ref[2]


def test_sharding_and_device_accumulation(engine):
    import torch
    from ba_amd import lib as L
    policy = A.SPLIT
    kw = dict(seed=SEEDS[1], f=10, **drawn(L))
    whole = engine.run_adv(10, 3, 256, policy, **kw)
    a = engine.run_adv(10, 3, 128, policy, **kw)
    b = engine.run_adv(10, 3, 128, policy, first_trial=128, **kw)
    same(np.concatenate([a.decisions, b.decisions]), whole.decisions, "decisions")
    same(np.concatenate([a.outcome, b.outcome]), whole.outcome, "outcome")
    assert {k: a.counters[k] + b.counters[k] for k in a.counters} == whole.counters
    check(whole, model(10, 3, policy, 256, SEEDS[1]), "whole")
    # the device entry accumulates into d_counters across calls
    cnt = torch.zeros(16, dtype=torch.int64, device="cuda")
    s = torch.cuda.current_stream().cuda_stream
    for first in (0, 128):
        engine.run_adv_device(L.make_params(10, 3, first_trial=first, **kw), 128, policy,
                              d_counters=cnt.data_ptr(), stream=s)
    torch.cuda.synchronize()
    assert dict(zip(L.COUNTER_NAMES, cnt.cpu().tolist())) == whole.counters
    assert cnt.cpu().tolist()[12:] == [0, 0, 0, 0]


def test_host_entry_chunks(engine, monkeypatch):
    """The host entry's chunk loop (forced small): same bits as one chunk."""
    from ba_amd import lib as L
    kw = dict(seed=SEEDS[0], f=10, **drawn(L))
    rng = np.random.default_rng(1)
    fm = rng.integers(0, 1 << 10, B, dtype=np.uint64).astype(np.uint32)
    oc = rng.choice([0, 1, 2], B).astype(np.uint8)
    one = engine.run_adv(10, 3, B, A.ANTI, **kw)
    one_g = engine.run_adv(10, 3, B, A.FLIP, faulty=fm, order=oc)
    monkeypatch.setenv("BA_ADV_HOST_CHUNK", "64")
    for ref, res in ((one, engine.run_adv(10, 3, B, A.ANTI, **kw)),
                     (one_g, engine.run_adv(10, 3, B, A.FLIP, faulty=fm, order=oc))):
        same(res.decisions, ref.decisions, "decisions")
        same(res.outcome, ref.outcome, "outcome")
        assert res.counters == ref.counters
    check(one, model(10, 3, A.ANTI, B, SEEDS[0]), "one chunk")


def test_errors(engine):
    from ba_amd import lib as L
    kw = dict(faulty_mode=L.FAULTY_EXACT, f=0, order_mode=L.ORDER_CONST)

    def code(**over):
        a = dict(n=4, m=1, batch=64, policy=A.SPLIT)
        a.update(kw)
        a.update(over)
        with pytest.raises(L.BAError) as e:
            engine.run_adv(a.pop("n"), a.pop("m"), a.pop("batch"), a.pop("policy"), **a)
        return e.value.code

    assert code(policy=3) == L.EINVAL
    assert code(policy=0xFFFFFFFF) == L.EINVAL
    assert code(lie_mode=L.LIE_TABLE) == L.ENOTSUP
    assert code(engine=L.ENGINE_FUSED) == L.EINVAL
    assert code(engine=L.ENGINE_LEVELS) == L.EINVAL
    assert code(n=0) == L.EINVAL
    assert code(n=33) == L.EINVAL
    assert code(m=9) == L.EINVAL
    assert code(first_trial=32) == L.EINVAL
    assert code(faulty_mode=L.FAULTY_GIVEN) == L.EINVAL  # no faulty_mask
    assert code(order_mode=L.ORDER_GIVEN) == L.EINVAL    # no order
    # the cap on a receiver's relay chains
    for n, m in ((32, 5), (16, 7), (16, 8)):
        assert code(n=n, m=m) == L.ETOOBIG
    # the device entry returns the same codes
    cnt = L.Counters()
    for p, policy, want in ((L.make_params(4, 1, **kw), 3, L.EINVAL),
                            (L.make_params(4, 1, lie_mode=L.LIE_TABLE, **kw), 0, L.ENOTSUP),
                            (L.make_params(4, 1, engine=L.ENGINE_LEVELS, **kw), 0, L.EINVAL),
                            (L.make_params(32, 5, **kw), 0, L.ETOOBIG)):
        rc = engine.lib.ba_adv_run_trials_device(engine.handle, ctypes.byref(p), policy, 64, None, None,
                                                 None, None, ctypes.addressof(cnt), None)
        assert rc == want
    # the trial index may not wrap: the last trial is at most 2^64 - 1
    with pytest.raises(L.BAError) as e:
        engine.run_adv(4, 1, 65, A.SPLIT, first_trial=2**64 - 64, **kw)
    assert e.value.code == L.EINVAL and "first_trial" in str(e.value)
    top = engine.run_adv(4, 1, 64, A.SPLIT, first_trial=2**64 - 64, **kw)  # ends at 2^64: valid
    dec, out, cnt = A.run(4, 1, A.SPLIT, first_trial=2**64 - 64, batch=64, **kw)
    check(top, (np.array(dec, np.uint64), np.array(out, np.uint8), cnt), "top")
    # batch = 0: BA_OK with zero counters
    res = engine.run_adv(4, 1, 0, A.SPLIT, **kw)
    assert all(v == 0 for v in res.counters.values())
    # the ctx still works
    assert engine.run_adv(4, 1, 64, A.SPLIT, **kw).counters["trials"] == 64


def test_cap_admits_the_largest_walks(engine):
    """(32, 4): 657,720 chains per receiver, the largest n under the cap, on one word."""
    from ba_amd import lib as L
    assert L.adv_paths(32, 4) == 657720
    fm = np.array([0, 1, 0b110, 0xFFFFFFFF], np.uint32)
    oc = np.array([1, 1, 0, 2], np.uint8)
    res = engine.run_adv(32, 4, 4, A.FLIP, faulty=fm, order=oc)
    c = res.counters
    assert c["trials"] == 4 and c["in_bound"] == 3 and c["bound_violations"] == 0
    assert res.decisions[0] == np.uint64(0x1555555555555555)  # no traitor: all 31 attack
    assert (int(res.outcome[2]) >> 2) & 1 and (int(res.outcome[2]) >> 4) & 1  # 2 <= 4 traitors of 32


@pytest.mark.parametrize("policy", A.POLICIES)
def test_bench_size_equals_sum_of_sixteen(engine, policy):
    """1,048,576 trials at (10, 3) in one call == sixteen 65,536-trial calls: 586
    blocks and the counter sink's replicas at bench size (a self-consistency check,
    not a model run)."""
    from ba_amd import lib as L
    kw = dict(seed=0xBA5EED, faulty_mode=L.FAULTY_RANDOM, f=3, order_mode=L.ORDER_RANDOM,
              want_decisions=False, want_outcome=False)
    T, K = 1 << 20, 16
    whole = engine.run_adv(10, 3, T, policy, **kw).counters
    tot = dict.fromkeys(whole, 0)
    for i in range(K):
        c = engine.run_adv(10, 3, T // K, policy, first_trial=i * (T // K), **kw).counters
        for k in tot:
            tot[k] += c[k]
    assert whole == tot
    assert whole["trials"] == T and whole["bound_violations"] == 0 and whole["in_bound"] == T


def test_persistent_block_loop_equals_shards(engine):
    """2,097,152 trials at (32, 1): 4,096 blocks of eight words, more than the grid's
    eight blocks per CU, so blocks take a second pass; sixteen 131,072-trial shards
    (512 blocks each) do not.  Decisions, outcome bytes and counters agree."""
    from ba_amd import lib as L
    kw = dict(seed=SEEDS[1], faulty_mode=L.FAULTY_RANDOM, f=32, order_mode=L.ORDER_RANDOM)
    T, K = 1 << 21, 16
    whole = engine.run_adv(32, 1, T, A.ANTI, **kw)
    parts = [engine.run_adv(32, 1, T // K, A.ANTI, first_trial=i * (T // K), **kw) for i in range(K)]
    same(whole.decisions, np.concatenate([p.decisions for p in parts]), "decisions")
    same(whole.outcome, np.concatenate([p.outcome for p in parts]), "outcome")
    assert whole.counters == {k: sum(p.counters[k] for p in parts) for k in whole.counters}
    ref = model(32, 1, A.ANTI, 70, SEEDS[1])  # the same draws: the first 70 trials against the model
    same(whole.decisions[:70], ref[0], "first 70 decisions")
    same(whole.outcome[:70], ref[1], "first 70 outcome")
