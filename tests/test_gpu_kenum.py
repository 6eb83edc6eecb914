"""GPU tests of the King enumeration (docs/SEMANTICS.md §11): k_kenum through the C ABI
against the two forms of the reference model (tests/kenum_model.py) and against the coin
and split engines k_king / k_king3.  Every comparison is exact: decisions, outcome bytes,
all 12 run counters and the witness."""
import ctypes
import functools

import numpy as np
import pytest

import ba_oracle as O
import kenum_model as M

pytestmark = pytest.mark.gpu

A, R, OTHER = O.ATTACK, O.RETREAT, O.OTHER
KING, KING3 = M.KING, M.KING3


# --- references (computed once, shared) ------------------------------------------------
@functools.lru_cache(maxsize=None)
def message(proto, n, m, F, o, first=0, count=None):
    if count is None:
        count = (1 << M.bits_formula(proto, n, m, F)) - first
    dec, out, cnt, wit = M.run_message(proto, n, m, F, o, first, count)
    return np.array(dec, np.uint64), np.array(out, np.uint8), cnt, wit


@functools.lru_cache(maxsize=None)
def space(proto, n, m, F):
    return M.Space(proto, n, m, F)


@functools.lru_cache(maxsize=None)
def plane(proto, n, m, F, o):
    return space(proto, n, m, F).run(o)


def same(a, b, what):
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape, f"{what}: shape {a.shape} != {b.shape}"
    if not np.array_equal(a, b):
        idx = np.nonzero(a != b)[0]
        raise AssertionError(f"{what}: {len(idx)} mismatches, first at {idx[:5].tolist()}: "
                             f"got {a[idx[:5]].tolist()} want {b[idx[:5]].tolist()}")


def check(res, ref, what):
    dec, out, cnt, wit = ref
    same(res.decisions, dec, f"{what} decisions")
    same(res.outcome, out, f"{what} outcome")
    assert len(cnt) == 12
    assert {k: res.counters[k] for k in cnt} == cnt, what
    assert res.witness == wit, what


def full(engine, proto, n, m, F, o, **kw):
    return engine.run_kenum(proto, n, m, F, o, want_decisions=True, want_outcome=True, **kw)


# --- 1. whole spaces against the message form -----------------------------------------
@pytest.mark.parametrize("o", [A, R, OTHER])
@pytest.mark.parametrize("F,B", [(0b0001, 12), (0b0010, 9)])
def test_king_whole_space_equals_message_form(engine, F, B, o):
    res = full(engine, KING, 4, 1, F, o)
    assert res.counters["trials"] == 1 << B
    check(res, message(KING, 4, 1, F, o), f"KING (4,1) F={F:#b} o={o}")


# --- 2. whole spaces against the plane form --------------------------------------------
@pytest.mark.parametrize("n,F,B,o", [(4, 0b0010, 21, A), (3, 0b001, 16, A), (3, 0b001, 16, R)])
def test_king3_whole_space_equals_plane_form(engine, n, F, B, o):
    """Counters and witness of the whole space; decisions and outcome bytes of 200
    strategies from a non-zero multiple of 64."""
    sp = space(KING3, n, 1, F)
    pref, cnt, wit = plane(KING3, n, 1, F, o)
    assert sp.B == B
    res = engine.run_kenum(KING3, n, 1, F, o)
    assert res.decisions is None and res.outcome is None
    assert {k: res.counters[k] for k in cnt} == cnt and res.witness == wit
    first = 64 * 37
    win = full(engine, KING3, n, 1, F, o, first=first, count=200)
    want = [sp.trial(pref, o, S) for S in range(first, first + 200)]
    same(win.decisions, np.array([w[0] for w in want], np.uint64), "window decisions")
    same(win.outcome, np.array([w[1] for w in want], np.uint8), "window outcome")


# --- 3. in bound: the theorems by exhaustion ---------------------------------------------
@pytest.mark.parametrize("o", [A, R])
@pytest.mark.parametrize("proto,n,m", [(KING, 5, 1), (KING3, 4, 1)])
def test_no_strategy_of_one_traitor_breaks_the_bound(engine, proto, n, m, o):
    from ba_amd import lib as L
    ran = 0
    for g in range(n):
        F = 1 << g
        B = L.kenum_bits(proto, n, m, F)
        if B > 24:
            continue
        ran += 1
        res = engine.run_kenum(proto, n, m, F, o)
        c = res.counters
        assert c["trials"] == 1 << B and c["in_bound"] == c["trials"], (F, c)  # the zero is not vacuous
        assert c["bound_violations"] == 0 and res.witness is None, (F, c, res.witness)
        assert c["agreement"] == c["trials"] and c["validity"] == c["validity_applicable"]
        assert c["validity_applicable"] == (0 if g == 0 else c["trials"])
        assert c["faulty_total"] == c["trials"] and c["undefined_decisions"] == 0
    assert ran == n  # every single-traitor set of both shapes has B <= 24


# --- 4. beyond the bound: the witness ------------------------------------------------------
@pytest.mark.parametrize("proto,n,m,F,o", [(KING, 4, 1, 0b0010, A), (KING, 4, 1, 0b0010, R),
                                           (KING3, 3, 1, 0b001, A), (KING3, 3, 1, 0b001, R)])
def test_witness_is_the_smallest_violating_strategy(engine, proto, n, m, F, o):
    from ba_amd import lib as L
    _, cnt, wit = plane(proto, n, m, F, o)
    res = engine.run_kenum(proto, n, m, F, o)
    assert wit is not None and res.witness == wit
    assert res.counters["agreement"] == cnt["agreement"] < cnt["trials"]
    assert res.counters["in_bound"] == 0 and res.counters["bound_violations"] == 0
    msgs = L.decode_kstrategy(proto, n, m, F, res.witness)
    assert msgs == M.messages_of(proto, n, m, F, res.witness)
    dec = M.history_message(proto, n, m, F, int(o == A), msgs)[-1][1:]
    assert M.violates(M.trial_outcome(proto, n, m, F, o, dec))
    # re-run as the last element of its word: nothing below it in the word violates
    first = wit & ~63
    one = full(engine, proto, n, m, F, o, first=first, count=wit - first + 1)
    assert one.witness == wit and M.violates(int(one.outcome[-1]))


# --- 5. ties to the coin and split engines -------------------------------------------------
# KING3 at (7,2) has no single-traitor case within 48 bits (54 at the least), so its
# second shape is (7,1), up to 48 bits.
TIES = [(KING, 5, 1), (KING, 7, 2), (KING3, 5, 1), (KING3, 7, 1)]


def test_king3_seven_two_is_above_the_bit_cap(engine):
    from ba_amd import lib as L
    assert min(L.kenum_bits(KING3, 7, 2, 1 << g) for g in range(7)) == 54
    assert max(L.kenum_bits(KING, 7, 2, 1 << g) for g in range(7)) <= 48
    with pytest.raises(L.BAError) as e:
        engine.run_kenum(KING3, 7, 2, 0b0001000, A, count=64)
    assert e.value.code == L.ETOOBIG


@pytest.mark.parametrize("proto,n,m", TIES)
def test_split_and_coin_trials_as_strategies_equal_the_engines(engine, proto, n, m):
    """What BA_KING_SPLIT, and each of 64 BA_KING_COIN trials of one seed, shows is one
    strategy S; k_kenum at S decides as k_king / k_king3 does in that trial: the loyal
    lieutenants' decision bits and the IC1 / IC2 flags."""
    from ba_amd import lib as L
    run = engine.run_king if proto == KING else engine.run_king3
    seed = 0x7E57ED
    for F in (0b1, 0b10, 1 << (n - 1)):
        loyal = sum(3 << (2 * (r - 1)) for r in range(1, n) if not (F >> r) & 1)
        for o in (A, R):
            kw = dict(seed=seed, faulty=[F] * 64, order=[o] * 64)
            cases = [("split", M.split_strategy(proto, n, m, F), run(n, m, 64, L.KING_SPLIT, **kw), 0)]
            coin = run(n, m, 64, L.KING_COIN, **kw)
            cases += [(f"coin {t}", M.coin_strategy(proto, n, m, F, seed, t), coin, t) for t in range(64)]
            for what, S, ref, t in cases:
                first = S & ~63
                got = full(engine, proto, n, m, F, o, first=first, count=64)
                i = S - first
                assert int(got.decisions[i]) & loyal == int(ref.decisions[t]) & loyal, (what, F, o)
                assert int(got.outcome[i]) & 0b11100 == int(ref.outcome[t]) & 0b11100, (what, F, o)


# --- 6. high index bits ----------------------------------------------------------------------
@pytest.mark.parametrize("first,count", [((1 << 48) - 4096, 4096), (1 << 38, 64 * 5 + 29)])
def test_high_bit_planes_and_the_64_bit_word_index(engine, first, count):
    """KING3 (7,1) F = {0}: 48 free bits, so bits up to 41 of the word index are planes."""
    from ba_amd import lib as L
    assert L.kenum_bits(KING3, 7, 1, 1) == 48
    for o in (A, R):
        check(full(engine, KING3, 7, 1, 1, o, first=first, count=count),
              message(KING3, 7, 1, 1, o, first, count), f"first={first} o={o}")


# --- 7. ranges ------------------------------------------------------------------------------
@pytest.mark.parametrize("proto,n,F", [(KING, 4, 0b0001), (KING3, 3, 0b001)])
def test_three_ranges_sum_to_the_whole_call(engine, proto, n, F):
    """Ends that are neither tile (4,096) nor word (64) aligned; B = 12 and 16."""
    T = (1 << 12) - 64 * 3 - 35
    cuts = [0, 64 * 7, 64 * 29, T]
    for o in (A, R):
        whole = engine.run_kenum(proto, n, 1, F, o, first=0, count=T)
        parts = [engine.run_kenum(proto, n, 1, F, o, first=a, count=b - a) for a, b in zip(cuts, cuts[1:])]
        assert whole.counters["trials"] == T
        assert whole.counters == {k: sum(p.counters[k] for p in parts) for k in whole.counters}
        wits = [p.witness for p in parts if p.witness is not None]
        assert whole.witness == (min(wits) if wits else None)
        assert {k: whole.counters[k] for k in O.COUNTERS} == message(proto, n, 1, F, o, 0, T)[2]


HIGH_FIRST = (1 << 41) | (1 << 33) | (64 * 77)  # a multiple of 64 with bits above 2^32


@pytest.mark.parametrize("proto,n,m,F,B,first", [(KING, 9, 2, 0b110000000, 42, 0), (KING3, 7, 1, 0b0001000, 36, 0),
                                                 (KING, 9, 2, 0b110000000, 42, HIGH_FIRST),
                                                 (KING, 7, 2, 0b1110000, 36, 1 << 33)])
def test_persistent_loop_counters_equal_single_pass_shards(engine, proto, n, m, F, B, first):
    """2^30 strategies in one call are 262,144 tiles: every wave of the grid (at most
    eight four-wave blocks per CU) takes tile after tile and carries its totals and its
    witness across them.  Thirty-two shards of 2^25 strategies (8,192 tiles, 2,048 blocks:
    one tile per wave on a 256-CU device) sum to the same counters, and the call's
    witness is the smallest of theirs.  The first three cases are in bound; KING (7,2)
    with three traitors is not: there a witness, if any, must lie in the range."""
    from ba_amd import lib as L
    assert L.kenum_bits(proto, n, m, F) == B
    T, K = 1 << 30, 32
    whole = engine.run_kenum(proto, n, m, F, A, first=first, count=T)
    parts = [engine.run_kenum(proto, n, m, F, A, first=first + i * (T // K), count=T // K) for i in range(K)]
    assert whole.counters == {k: sum(p.counters[k] for p in parts) for k in whole.counters}
    wits = [p.witness for p in parts if p.witness is not None]
    assert whole.witness == (min(wits) if wits else None)
    c = whole.counters
    assert c["trials"] == T
    clean = c["agreement"] == T and c["validity"] == c["validity_applicable"]
    assert (whole.witness is None) == clean
    if (proto, n) == (KING, 7):
        assert c["in_bound"] == 0 and (clean or first <= whole.witness < first + T)
    else:
        assert c["in_bound"] == T and c["bound_violations"] == 0 and clean


def test_persistent_loop_with_outputs_equals_single_pass_shards(engine):
    """With per-trial outputs the blocks are one wave each, at most 32 per CU.  One device
    call of 2^26 + 4,096 + 229 strategies is 16,386 tiles, so blocks take a second and a
    third tile and reuse their decision planes in LDS; the same range as calls of 2^24
    (4,096 tiles each: one tile per block) gives the same bytes, counters and witness, and
    the range's two ends (a whole tile; a tile and a partial word) equal the model."""
    import torch
    from ba_amd import lib as L
    proto, n, m, F, o, first = KING3, 7, 1, 0b0001000, A, 1 << 35
    assert L.kenum_bits(proto, n, m, F) == 36
    T, S = (1 << 26) + 4096 + 229, 1 << 24
    s = torch.cuda.current_stream().cuda_stream

    def run(lo, count, dec, out, cnt, wit):
        engine.run_kenum_device(L.make_params(n, m, first_trial=first + lo), proto, F, o, count,
                                d_decisions=dec[lo:].data_ptr(), d_outcome=out[lo:].data_ptr(),
                                d_counters=cnt.data_ptr(), d_witness=wit.data_ptr(), stream=s)

    bufs = []
    for shard in (T, S):
        dec = torch.full((T,), -1, dtype=torch.int64, device="cuda")
        out = torch.full((T,), 255, dtype=torch.uint8, device="cuda")
        cnt = torch.zeros(16, dtype=torch.int64, device="cuda")
        wit = torch.full((1,), -1, dtype=torch.int64, device="cuda")
        for lo in range(0, T, shard):
            run(lo, min(shard, T - lo), dec, out, cnt, wit)
        torch.cuda.synchronize()
        bufs.append((dec, out, cnt, wit))
    (dec, out, cnt, wit), ref = bufs
    assert torch.equal(dec, ref[0]) and torch.equal(out, ref[1])
    assert torch.equal(cnt, ref[2]) and torch.equal(wit, ref[3])
    assert int(cnt[0]) == T and cnt.cpu().tolist()[12:] == [0, 0, 0, 0]
    for lo, count in ((0, 4096), (T - 4096 - 229, 4096 + 229)):
        mdec, mout, _, _ = message(proto, n, m, F, o, first + lo, count)
        same(dec[lo:lo + count].cpu().numpy().view(np.uint64), mdec, f"decisions at {lo}")
        same(out[lo:lo + count].cpu().numpy(), mout, f"outcome at {lo}")
    c = dict(zip(L.COUNTER_NAMES, cnt.cpu().tolist()))
    clean = c["agreement"] == T and c["validity"] == c["validity_applicable"]
    assert (int(wit.cpu().numpy().view(np.uint64)[0]) == L.NO_WITNESS) == clean


def test_host_chunks_give_identical_outputs(engine, monkeypatch):
    first, count = 64 * 2, 64 * 9 + 17
    ref = message(KING3, 3, 1, 0b001, A, first, count)
    one = full(engine, KING3, 3, 1, 0b001, A, first=first, count=count)
    monkeypatch.setenv("BA_KENUM_HOST_CHUNK", "128")
    chunked = full(engine, KING3, 3, 1, 0b001, A, first=first, count=count)
    only = engine.run_kenum(KING3, 3, 1, 0b001, A, first=first, count=count, want_outcome=True)
    monkeypatch.delenv("BA_KENUM_HOST_CHUNK")
    for res in (one, chunked):
        check(res, ref, "host path")
    assert only.decisions is None and only.counters == one.counters and only.witness == one.witness
    same(only.outcome, ref[1], "outcome alone")


def test_device_entry_accumulates_counters_and_min_accumulates_the_witness(engine):
    import torch
    from ba_amd import lib as L
    ref = message(KING, 4, 1, 0b0010, R)
    cnt = torch.zeros(16, dtype=torch.int64, device="cuda")
    wit = torch.full((1,), -1, dtype=torch.int64, device="cuda")  # 2^64 - 1
    s = torch.cuda.current_stream().cuda_stream
    for first in (256, 0):  # the second call lowers the witness
        engine.run_kenum_device(L.make_params(4, 1, first_trial=first), KING, 0b0010, R, 256,
                                d_counters=cnt.data_ptr(), d_witness=wit.data_ptr(), stream=s)
        torch.cuda.synchronize()
        lo = [t for t in range(first, 512) if M.violates(int(ref[1][t]))][0]
        assert int(wit.cpu().numpy().view(np.uint64)[0]) == lo
    assert dict(zip(L.COUNTER_NAMES, cnt.cpu().tolist())) == ref[2]
    assert cnt.cpu().tolist()[12:] == [0, 0, 0, 0]
    assert int(wit.cpu().numpy().view(np.uint64)[0]) == ref[3] == 144


# --- 8. errors ----------------------------------------------------------------------------------
def test_errors(engine):
    from ba_amd import lib as L

    def code(proto=KING, n=4, m=1, F=0b0010, o=A, **kw):
        with pytest.raises(L.BAError) as e:
            engine.run_kenum(proto, n, m, F, o, **kw)
        return e.value.code

    assert code(first=0, count=513) == L.EINVAL            # past 2^9
    assert code(first=512, count=1) == L.EINVAL
    assert code(first=32, count=1) == L.EINVAL             # not a multiple of 64
    assert code(o=3) == L.EINVAL
    assert code(proto=2, count=1) == L.EINVAL
    assert code(lie_mode=L.LIE_TABLE) == L.ENOTSUP
    assert code(engine=L.ENGINE_FUSED) == L.EINVAL
    assert code(engine=L.ENGINE_LEVELS) == L.EINVAL
    assert code(faulty_mode=L.FAULTY_RANDOM) == L.EINVAL
    assert code(faulty_mode=L.FAULTY_EXACT) == L.EINVAL
    assert code(order_mode=L.ORDER_RANDOM) == L.EINVAL
    assert code(order_mode=L.ORDER_CONST) == L.EINVAL
    assert code(n=0, count=1) == L.EINVAL
    assert code(n=33, count=1) == L.EINVAL
    assert code(proto=KING, m=9, count=1) == L.EINVAL
    assert code(proto=KING3, m=11, count=1) == L.EINVAL
    assert code(n=17, m=0, count=64) == L.ETOOBIG          # 16 bits, but n > 16
    assert code(n=32, m=0, count=64) == L.ETOOBIG
    assert code(proto=KING3, n=7, m=2, count=64) == L.ETOOBIG   # 60 bits
    assert code(n=16, m=8, F=0b1, count=64) == L.ETOOBIG        # 165 bits
    # m = 9 and 10 are KING3's own
    res = engine.run_kenum(KING3, 4, 10, 0b0010, A, first=0, count=64)
    assert res.counters["trials"] == 64 and L.kenum_bits(KING3, 4, 10, 0b0010) == 39
    # the device entry returns the same codes
    cnt = L.Counters()

    def dcode(p, proto=KING, F=0b0010, o=A, count=16):
        return engine.lib.ba_kenum_run_device(engine.handle, ctypes.byref(p), proto, F, o, count, None,
                                              None, ctypes.addressof(cnt), None, None)

    assert dcode(L.make_params(4, 1), count=513) == L.EINVAL
    assert dcode(L.make_params(4, 1, first_trial=32), count=1) == L.EINVAL
    assert dcode(L.make_params(4, 1), o=3) == L.EINVAL
    assert dcode(L.make_params(4, 1), proto=2) == L.EINVAL
    assert dcode(L.make_params(4, 1, lie_mode=L.LIE_TABLE)) == L.ENOTSUP
    assert dcode(L.make_params(4, 1, engine=L.ENGINE_LEVELS)) == L.EINVAL
    assert dcode(L.make_params(4, 1, faulty_mode=L.FAULTY_EXACT)) == L.EINVAL
    assert dcode(L.make_params(4, 1, order_mode=L.ORDER_CONST)) == L.EINVAL
    assert dcode(L.make_params(0, 1)) == L.EINVAL
    assert dcode(L.make_params(33, 1)) == L.EINVAL
    assert dcode(L.make_params(4, 9)) == L.EINVAL
    assert dcode(L.make_params(4, 11), proto=KING3) == L.EINVAL
    assert dcode(L.make_params(17, 0)) == L.ETOOBIG
    assert dcode(L.make_params(7, 2), proto=KING3) == L.ETOOBIG
    assert engine.lib.ba_kenum_run_device(engine.handle, ctypes.byref(L.make_params(4, 1)), KING, 0b0010, A,
                                          16, None, None, None, None, None) == L.EINVAL  # no d_counters
    assert engine.lib.ba_kenum_run_device(None, ctypes.byref(L.make_params(4, 1)), KING, 0b0010, A, 16,
                                          None, None, ctypes.addressof(cnt), None, None) == L.EINVAL
    # count = 0: BA_OK with zero counters and no witness
    res = engine.run_kenum(KING, 4, 1, 0b0010, A, count=0)
    assert all(v == 0 for v in res.counters.values()) and res.witness is None
    # F = 0: a space of one strategy, nobody lies
    res = full(engine, KING3, 4, 1, 0, A)
    assert res.counters["trials"] == 1 and res.counters["validity"] == 1 and res.witness is None
    assert int(res.decisions[0]) == 0b010101
    # the ctx still works
    check(full(engine, KING, 4, 1, 0b0010, A), message(KING, 4, 1, 0b0010, A), "after the errors")


# --- 9. graph capture ------------------------------------------------------------------------------
def test_device_entry_is_captured_in_a_graph_and_replayed():
    """ba_kenum_run_device copies nothing from the host, so a capturing stream takes it
    (ba_enum_run_device refuses): an eager call on a ctx of its own, the same call
    captured, two replays with counters and witness reset; each equals the model."""
    import torch
    from ba_amd import lib as L
    proto, n, m, F, o, T = KING, 4, 1, 0b0010, R, 512
    ref = message(proto, n, m, F, o)
    eng = L.Engine(0)
    try:
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            dec = torch.full((T,), -1, dtype=torch.int64, device="cuda")
            out = torch.full((T,), 255, dtype=torch.uint8, device="cuda")
            cnt = torch.zeros(16, dtype=torch.int64, device="cuda")
            wit = torch.full((1,), -1, dtype=torch.int64, device="cuda")

        def issue():
            eng.run_kenum_device(L.make_params(n, m), proto, F, o, T, d_decisions=dec.data_ptr(),
                                 d_outcome=out.data_ptr(), d_counters=cnt.data_ptr(),
                                 d_witness=wit.data_ptr(), stream=s.cuda_stream)

        def reset():
            with torch.cuda.stream(s):
                dec.fill_(-1)
                out.fill_(255)
                cnt.zero_()
                wit.fill_(-1)

        def verify(what):
            torch.cuda.synchronize()
            same(dec.cpu().numpy().view(np.uint64), ref[0], f"{what} decisions")
            same(out.cpu().numpy(), ref[1], f"{what} outcome")
            assert dict(zip(L.COUNTER_NAMES, cnt.cpu().tolist())) == ref[2], what
            assert cnt.cpu().tolist()[12:] == [0, 0, 0, 0], what
            assert int(wit.cpu().numpy().view(np.uint64)[0]) == ref[3], what

        issue()
        verify("eager")
        reset()
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            issue()
        for k in (1, 2):
            reset()
            with torch.cuda.stream(s):
                g.replay()
            verify(f"replay {k}")
        reset()
        issue()
        verify("eager after the replays")
        del g
    finally:
        torch.cuda.synchronize()
        eng.close()
