"""GPU tests of the RAND enumeration (docs/SEMANTICS.md §14): k_renum through the C ABI
against the two forms of the reference model (tests/renum_model.py) and against k_rand.
Every comparison is exact: decisions, outcome bytes, `decided` bytes, all 12 run
counters, the witness and the stats."""
import ctypes
import functools

import numpy as np
import pytest

import ba_oracle as O
import rand_model as RM
import renum_model as M

pytestmark = pytest.mark.gpu

A, R, OTHER = O.ATTACK, O.RETREAT, O.OTHER
LOCAL, COMMON = M.LOCAL, M.COMMON


# --- references (computed once, shared) ------------------------------------------------
@functools.lru_cache(maxsize=None)
def message(coin, n, m, R_, F, o, first=0, count=None):
    if count is None:
        count = (1 << M.bits_formula(coin, n, m, R_, F)) - first
    dec, out, dcd, cnt, wit, st = M.run_message(coin, n, m, R_, F, o, first, count)
    return np.array(dec, np.uint64), np.array(out, np.uint8), np.array(dcd, np.uint8), cnt, wit, st


@functools.lru_cache(maxsize=None)
def space(coin, n, m, R_, F):
    return M.Space(coin, n, m, R_, F)


@functools.lru_cache(maxsize=None)
def plane(coin, n, m, R_, F, o):
    return space(coin, n, m, R_, F).run(o)


def same(a, b, what):
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape, f"{what}: shape {a.shape} != {b.shape}"
    if not np.array_equal(a, b):
        idx = np.nonzero(a != b)[0]
        raise AssertionError(f"{what}: {len(idx)} mismatches, first at {idx[:5].tolist()}: "
                             f"got {a[idx[:5]].tolist()} want {b[idx[:5]].tolist()}")


def check_totals(res, cnt, wit, st, what):
    assert len(cnt) == 12
    assert {k: res.counters[k] for k in cnt} == cnt, what
    assert res.witness == wit, what
    assert res.stats == st, (what, res.stats, st)
    assert st["unsafe"] + st["undecided"] + sum(st["decided_in"]) == cnt["trials"], what


def check(res, ref, what):
    dec, out, dcd, cnt, wit, st = ref
    same(res.decisions, dec, f"{what} decisions")
    same(res.outcome, out, f"{what} outcome")
    same(res.decided, dcd, f"{what} decided")
    check_totals(res, cnt, wit, st, what)


def full(engine, coin, n, m, R_, F, o, **kw):
    return engine.run_renum(coin, n, m, R_, F, o, want_decisions=True, want_outcome=True, want_decided=True,
                            **kw)


def stats_of(words):
    from ba_amd import lib as L
    return L.renum_stats(np.asarray(words.cpu()).view(np.uint64))


def add_stats(parts):
    st = M.new_stats()
    for p in parts:
        st["unsafe"] += p["unsafe"]
        st["undecided"] += p["undecided"]
        st["decided_in"] = [a + b for a, b in zip(st["decided_in"], p["decided_in"])]
        for k in ("unsafe_witness", "undecided_witness"):
            both = [v for v in (st[k], p[k]) if v is not None]
            st[k] = min(both) if both else None
    return st


# --- 1. whole spaces against the message form -----------------------------------------
@pytest.mark.parametrize("o", [A, R, OTHER])
@pytest.mark.parametrize("coin,B", [(LOCAL, 12), (COMMON, 10)])
def test_one_faulty_lieutenant_whole_space_equals_message_form(engine, coin, B, o):
    res = full(engine, coin, 4, 1, 1, 0b0010, o)
    assert res.counters["trials"] == 1 << B
    check(res, message(coin, 4, 1, 1, 0b0010, o), f"(4,1) R=1 F={{1}} coin={coin} o={o}")


@pytest.mark.parametrize("coin,n,R_,F,o,B", [(LOCAL, 4, 1, 0b0001, A, 15), (COMMON, 4, 1, 0b0001, R, 13),
                                             (LOCAL, 3, 2, 0b010, A, 16), (COMMON, 3, 2, 0b010, R, 14),
                                             (COMMON, 3, 2, 0b001, A, 16)])
def test_whole_space_equals_message_form(engine, coin, n, R_, F, o, B):
    res = full(engine, coin, n, 1, R_, F, o)
    assert res.counters["trials"] == 1 << B
    check(res, message(coin, n, 1, R_, F, o), f"({n},1) R={R_} F={F:#b} coin={coin} o={o}")


def test_three_one_faulty_commander_local_two_phases(engine):
    """(3,1) R=2 LOCAL F={0}, attack: 2^18 strategies.  The stats are the message form's
    recorded figures (first unsafe S = 63, decided {1: 1040, 2: 2880, 254: 4848, 255:
    253376}; tests/test_renum_model.py holds the plane form to the same figures), the
    counters the plane form's, and a 200-strategy window is the message form's."""
    coin, n, R_, F, o = LOCAL, 3, 2, 0b001, A
    _, _, cnt, wit, st = plane(coin, n, 1, R_, F, o)
    assert (st["decided_in"][1], st["decided_in"][2], st["unsafe"], st["undecided"]) == (1040, 2880, 4848, 253376)
    assert st["unsafe_witness"] == 63
    res = engine.run_renum(coin, n, 1, R_, F, o)
    assert res.decisions is None and res.outcome is None and res.decided is None
    check_totals(res, cnt, wit, st, "2^18")
    first = 64 * 1021
    check(full(engine, coin, n, 1, R_, F, o, first=first, count=200),
          message(coin, n, 1, R_, F, o, first, 200), "window")


# --- 2. whole spaces against the plane form --------------------------------------------
@pytest.mark.parametrize("coin,n,R_,F,B,o", [(LOCAL, 4, 2, 0b0010, 24, A), (COMMON, 4, 2, 0b0100, 20, R),
                                             (LOCAL, 4, 1, 0b0110, 14, A), (COMMON, 3, 3, 0b100, 21, R)])
def test_whole_space_equals_plane_form(engine, coin, n, R_, F, B, o):
    """Counters, witness and stats of the whole space; decisions, outcome and decided
    bytes of 200 strategies from a non-zero multiple of 64."""
    sp = space(coin, n, 1, R_, F)
    x, dpl, cnt, wit, st = plane(coin, n, 1, R_, F, o)
    assert sp.B == B
    res = engine.run_renum(coin, n, 1, R_, F, o)
    check_totals(res, cnt, wit, st, "whole space")
    first = 64 * 37
    win = full(engine, coin, n, 1, R_, F, o, first=first, count=200)
    want = [sp.trial(x, dpl, o, S) for S in range(first, first + 200)]
    same(win.decisions, np.array([w[0] for w in want], np.uint64), "window decisions")
    same(win.outcome, np.array([w[1] for w in want], np.uint8), "window outcome")
    same(win.decided, np.array([w[2] for w in want], np.uint8), "window decided")


# --- 3. in bound: safety by exhaustion -----------------------------------------------------
@pytest.mark.parametrize("o", [A, R])
@pytest.mark.parametrize("coin", [LOCAL, COMMON])
@pytest.mark.parametrize("R_", [1, 2])
def test_no_play_of_one_traitor_is_unsafe_in_bound(engine, R_, coin, o):
    from ba_amd import lib as L
    n, m, ran = 4, 1, 0
    for g in range(n):
        F = 1 << g
        B = L.renum_bits(coin, n, m, R_, F)
        if B > 28:
            continue
        ran += 1
        res = engine.run_renum(coin, n, m, R_, F, o)
        c, st = res.counters, res.stats
        assert c["trials"] == 1 << B and c["in_bound"] == c["trials"], (F, c)  # the zero is not vacuous
        assert st["unsafe"] == 0 and st["unsafe_witness"] is None, (F, st)
        assert st["undecided"] + sum(st["decided_in"]) == c["trials"]
        if g != 0:
            assert st["decided_in"][1] == c["trials"] and c["bound_violations"] == 0, (F, st, c)
            assert c["validity"] == c["validity_applicable"] == c["trials"]
    # R = 2 with a faulty commander is 27 (LOCAL) / 21 (COMMON) bits; lieutenants 24 / 20
    assert ran == n


# --- 4. beyond the bound: the witness ------------------------------------------------------
@pytest.mark.parametrize("coin,F,o", [(LOCAL, 0b010, A), (LOCAL, 0b010, R), (COMMON, 0b010, R), (COMMON, 0b001, A)])
def test_unsafe_witness_is_the_smallest_unsafe_strategy(engine, coin, F, o):
    from ba_amd import lib as L
    n, m, R_ = 3, 1, 2
    want = message(coin, n, m, R_, F, o)
    res = engine.run_renum(coin, n, m, R_, F, o)
    S = res.stats["unsafe_witness"]
    assert S is not None and S == want[5]["unsafe_witness"] and res.stats["unsafe"] == want[5]["unsafe"] > 0
    assert res.counters["in_bound"] == 0 and res.counters["bound_violations"] == 0
    play = L.decode_rstrategy(coin, n, m, R_, F, S)
    assert play == M.messages_of(coin, n, m, R_, F, S)
    # replayed through rand_model.phase_step
    msgs, coins = play["messages"], play["coins"]
    ob = int(o == A)
    faulty = lambda g: (F >> g) & 1  # noqa: E731
    x = RM.round0(n, F, ob, lambda r: 0 if faulty(r) else msgs[(0, 0, r)])
    D, V, unsafe = [0] * n, [0] * n, False
    for p in range(1, R_ + 1):
        x, D, V = RM.phase_step(
            n, m, F, x, D, V, lambda j, i: 0 if faulty(i) else msgs[(3 * p - 2, j, i)],
            lambda j, i: None if faulty(i) else msgs[(3 * p - 1, j, i)],
            lambda i: coins[(p, None)] if coin == COMMON else (0 if faulty(i) else coins[(p, i)]))
        unsafe = unsafe or RM.unsafe_state(n, F, ob, x, D, V)
    assert unsafe
    # re-run as the last element of its word: nothing below it in the word is unsafe
    first = S & ~63
    one = full(engine, coin, n, m, R_, F, o, first=first, count=S - first + 1)
    assert one.stats["unsafe_witness"] == S and int(one.decided[-1]) == M.UNSAFE
    assert list(one.decided[:-1]).count(M.UNSAFE) == 0 and one.stats["unsafe"] == 1


# --- 5. the tie to k_rand ------------------------------------------------------------------
@pytest.mark.parametrize("coin", [LOCAL, COMMON])
@pytest.mark.parametrize("n,m,R_,F", [(4, 1, 3, 0b0001), (4, 1, 3, 0b0100), (5, 1, 2, 0b00010),
                                      (7, 2, 1, 0b0000110)])
def test_rand_trials_as_strategies_equal_k_rand(engine, coin, n, m, R_, F):
    """Each of 64 BA_KING_COIN trials of one seed, and the BA_KING_SPLIT trial 0, is one
    strategy S (§14's map); k_renum at S gives the loyal lieutenants' decision bits, the
    IC1 / IC2 flags and the `decided` byte that k_rand gives in that trial."""
    from ba_amd import lib as L
    seed = 0x7E57ED
    loyal = sum(3 << (2 * (r - 1)) for r in range(1, n) if not (F >> r) & 1)
    assert L.renum_bits(coin, n, m, R_, F) <= 48
    for o in (A, R):
        kw = dict(coin=coin, seed=seed, faulty=[F] * 64, order=[o] * 64, want_decided=True)
        split = engine.run_rand(n, m, 64, R_, policy=L.KING_SPLIT, **kw)
        coinr = engine.run_rand(n, m, 64, R_, policy=L.KING_COIN, **kw)
        cases = [("split", M.split_strategy(coin, n, m, R_, F, seed, 0), split, 0)]
        cases += [(f"coin {t}", M.coin_strategy(coin, n, m, R_, F, seed, t), coinr, t) for t in range(64)]
        for what, S, ref, t in cases:
            first = S & ~63
            got = full(engine, coin, n, m, R_, F, o, first=first, count=64)
            i = S - first
            assert int(got.decisions[i]) & loyal == int(ref.decisions[t]) & loyal, (what, o)
            assert int(got.outcome[i]) & 0b11100 == int(ref.outcome[t]) & 0b11100, (what, o)
            assert int(got.decided[i]) == int(ref.decided[t]), (what, o)


# --- 6. high index bits ----------------------------------------------------------------------
@pytest.mark.parametrize("first,count", [((1 << 48) - 4096, 4096), (1 << 38, 64 * 5 + 29)])
def test_high_bit_planes_and_the_64_bit_word_index(engine, first, count):
    """(5,1) R=3 LOCAL F = {2}: 48 free bits, so bits up to 41 of the word index are planes."""
    from ba_amd import lib as L
    assert L.renum_bits(LOCAL, 5, 1, 3, 0b00100) == 48
    for o in (A, R):
        check(full(engine, LOCAL, 5, 1, 3, 0b00100, o, first=first, count=count),
              message(LOCAL, 5, 1, 3, 0b00100, o, first, count), f"first={first} o={o}")


# --- 7. ranges ------------------------------------------------------------------------------
@pytest.mark.parametrize("coin,F,o", [(COMMON, 0b010, R), (LOCAL, 0b010, A)])
def test_three_ranges_sum_to_the_whole_call(engine, coin, F, o):
    """Ends that are neither tile (4,096) nor word (64) aligned; B = 14 and 16."""
    T = (1 << 12) - 64 * 3 - 35
    cuts = [0, 64 * 7, 64 * 29, T]
    whole = engine.run_renum(coin, 3, 1, 2, F, o, first=0, count=T)
    parts = [engine.run_renum(coin, 3, 1, 2, F, o, first=a, count=b - a) for a, b in zip(cuts, cuts[1:])]
    assert whole.counters["trials"] == T
    assert whole.counters == {k: sum(p.counters[k] for p in parts) for k in whole.counters}
    wits = [p.witness for p in parts if p.witness is not None]
    assert whole.witness == (min(wits) if wits else None)
    assert whole.stats == add_stats([p.stats for p in parts])
    ref = message(coin, 3, 1, 2, F, o, 0, T)
    check_totals(whole, ref[3], ref[4], ref[5], "whole")


HIGH_FIRST = (1 << 38) | (1 << 33) | (64 * 77)  # a multiple of 64 with bits above 2^32


@pytest.mark.parametrize("coin,n,m,R_,F,B,first", [(LOCAL, 7, 2, 1, 0b0000110, 35, 0),
                                                   (LOCAL, 4, 1, 3, 0b0001, 39, HIGH_FIRST),
                                                   (COMMON, 3, 1, 4, 0b010, 28, 0)])
def test_persistent_loop_totals_equal_single_pass_shards(engine, coin, n, m, R_, F, B, first):
    """2^30 strategies in one call are 262,144 tiles: every wave of the grid takes tile
    after tile and carries its totals and its three witnesses across them.  Thirty-two
    shards of 2^25 strategies sum to the same counters and stat counts, and the call's
    witnesses are the smallest of theirs.  The first two cases are in bound (nothing
    unsafe); (3,1) is not, and takes its whole space of 2^28."""
    from ba_amd import lib as L
    assert L.renum_bits(coin, n, m, R_, F) == B
    T, K = min(1 << 30, 1 << B), 32
    whole = engine.run_renum(coin, n, m, R_, F, A, first=first, count=T)
    parts = [engine.run_renum(coin, n, m, R_, F, A, first=first + i * (T // K), count=T // K) for i in range(K)]
    assert whole.counters == {k: sum(p.counters[k] for p in parts) for k in whole.counters}
    wits = [p.witness for p in parts if p.witness is not None]
    assert whole.witness == (min(wits) if wits else None)
    assert whole.stats == add_stats([p.stats for p in parts])
    c, st = whole.counters, whole.stats
    assert c["trials"] == T == st["unsafe"] + st["undecided"] + sum(st["decided_in"])
    for k in ("unsafe_witness", "undecided_witness"):
        assert st[k] is None or first <= st[k] < first + T
    if n == 3:
        assert c["in_bound"] == 0 and st["unsafe"] > 0 and st["unsafe_witness"] is not None
    else:
        assert c["in_bound"] == T and st["unsafe"] == 0 and st["unsafe_witness"] is None


def test_persistent_loop_with_outputs_equals_single_pass_shards(engine):
    """With per-trial outputs the blocks are one wave each.  One device call of 2^26 + 4,096
    + 229 strategies is 16,386 tiles, so blocks take a second and a third tile and reuse
    their decision planes in LDS; the same range as calls of 2^24 gives the same bytes,
    counters, witness and stats, and the range's two ends equal the model."""
    import torch
    from ba_amd import lib as L
    coin, n, m, R_, F, o, first = LOCAL, 7, 2, 1, 0b0000110, A, 1 << 34
    assert L.renum_bits(coin, n, m, R_, F) == 35
    T, S = (1 << 26) + 4096 + 229, 1 << 24
    s = torch.cuda.current_stream().cuda_stream

    def run(lo, count, dec, out, dcd, cnt, wit, sts):
        engine.run_renum_device(L.make_params(n, m, first_trial=first + lo), coin, R_, F, o, count,
                                d_decisions=dec[lo:].data_ptr(), d_outcome=out[lo:].data_ptr(),
                                d_decided=dcd[lo:].data_ptr(), d_counters=cnt.data_ptr(),
                                d_witness=wit.data_ptr(), d_stats=sts.data_ptr(), stream=s)

    bufs = []
    for shard in (T, S):
        dec = torch.full((T,), -1, dtype=torch.int64, device="cuda")
        out = torch.full((T,), 255, dtype=torch.uint8, device="cuda")
        dcd = torch.full((T,), 77, dtype=torch.uint8, device="cuda")
        cnt = torch.zeros(16, dtype=torch.int64, device="cuda")
        wit = torch.full((1,), -1, dtype=torch.int64, device="cuda")
        sts = torch.zeros(L.RENUM_NSTATS, dtype=torch.int64, device="cuda")
        sts[2:4] = -1
        for lo in range(0, T, shard):
            run(lo, min(shard, T - lo), dec, out, dcd, cnt, wit, sts)
        torch.cuda.synchronize()
        bufs.append((dec, out, dcd, cnt, wit, sts))
    got, ref = bufs
    for a, b in zip(got, ref):
        assert torch.equal(a, b)
    dec, out, dcd, cnt, wit, sts = got
    assert int(cnt[0]) == T and cnt.cpu().tolist()[12:] == [0, 0, 0, 0]
    st = stats_of(sts)
    assert st["unsafe"] + st["undecided"] + sum(st["decided_in"]) == T
    for lo, count in ((0, 4096), (T - 4096 - 229, 4096 + 229)):
        mdec, mout, mdcd, _, _, _ = message(coin, n, m, R_, F, o, first + lo, count)
        same(dec[lo:lo + count].cpu().numpy().view(np.uint64), mdec, f"decisions at {lo}")
        same(out[lo:lo + count].cpu().numpy(), mout, f"outcome at {lo}")
        same(dcd[lo:lo + count].cpu().numpy(), mdcd, f"decided at {lo}")


def test_host_chunks_give_identical_outputs(engine, monkeypatch):
    coin, n, R_, F, o = LOCAL, 3, 2, 0b010, A
    first, count = 64 * 2, 64 * 9 + 17
    ref = message(coin, n, 1, R_, F, o, first, count)
    one = full(engine, coin, n, 1, R_, F, o, first=first, count=count)
    monkeypatch.setenv("BA_RENUM_HOST_CHUNK", "128")
    chunked = full(engine, coin, n, 1, R_, F, o, first=first, count=count)
    only = engine.run_renum(coin, n, 1, R_, F, o, first=first, count=count, want_decided=True)
    monkeypatch.delenv("BA_RENUM_HOST_CHUNK")
    for res in (one, chunked):
        check(res, ref, "host path")
    assert only.decisions is None and only.outcome is None
    assert only.counters == one.counters and only.witness == one.witness and only.stats == one.stats
    same(only.decided, ref[2], "decided alone")


# --- 8. device entry --------------------------------------------------------------------------
def test_device_entry_accumulates_and_min_accumulates_its_three_witnesses(engine):
    import torch
    from ba_amd import lib as L
    coin, n, m, R_, F, o = COMMON, 3, 1, 2, 0b010, R
    ref = message(coin, n, m, R_, F, o)
    dcd_ref, out_ref = ref[2], ref[1]
    lo_first, hi_first, span = 0, 4096, 4096
    cnt = torch.zeros(16, dtype=torch.int64, device="cuda")
    wit = torch.full((1,), -1, dtype=torch.int64, device="cuda")  # 2^64 - 1
    sts = torch.zeros(L.RENUM_NSTATS, dtype=torch.int64, device="cuda")
    sts[2:4] = -1
    s = torch.cuda.current_stream().cuda_stream
    seen = []
    for first in (hi_first, lo_first):  # the second call lowers the witnesses
        engine.run_renum_device(L.make_params(n, m, first_trial=first), coin, R_, F, o, span,
                                d_counters=cnt.data_ptr(), d_witness=wit.data_ptr(), d_stats=sts.data_ptr(),
                                stream=s)
        torch.cuda.synchronize()
        seen += list(range(first, first + span))
        st = stats_of(sts)
        low = lambda pred: min((t for t in seen if pred(t)), default=None)  # noqa: E731
        assert st["unsafe_witness"] == low(lambda t: dcd_ref[t] == M.UNSAFE)
        assert st["undecided_witness"] == low(lambda t: dcd_ref[t] == M.UNDECIDED)
        w = int(wit.cpu().numpy().view(np.uint64)[0])
        assert (None if w == L.NO_WITNESS else w) == low(lambda t: M.violates(int(out_ref[t])))
        assert st["unsafe"] == sum(1 for t in seen if dcd_ref[t] == M.UNSAFE)
        assert st["decided_in"][1] == sum(1 for t in seen if dcd_ref[t] == 1)
    want = message(coin, n, m, R_, F, o, 0, 2 * span)
    assert dict(zip(L.COUNTER_NAMES, cnt.cpu().tolist())) == want[3]
    assert cnt.cpu().tolist()[12:] == [0, 0, 0, 0]
    assert stats_of(sts) == want[5] and want[5]["unsafe_witness"] == 1985


def test_device_entry_is_captured_in_a_graph_and_replayed():
    """ba_renum_run_device copies nothing from the host, so a capturing stream takes it: an
    eager call on a ctx of its own, the same call captured, two replays with every
    accumulated word reset; each equals the model."""
    import torch
    from ba_amd import lib as L
    coin, n, m, R_, F, o, T = LOCAL, 4, 1, 1, 0b0010, R, 4096
    ref = message(coin, n, m, R_, F, o)
    eng = L.Engine(0)
    try:
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            dec = torch.full((T,), -1, dtype=torch.int64, device="cuda")
            out = torch.full((T,), 255, dtype=torch.uint8, device="cuda")
            dcd = torch.full((T,), 77, dtype=torch.uint8, device="cuda")
            cnt = torch.zeros(16, dtype=torch.int64, device="cuda")
            wit = torch.full((1,), -1, dtype=torch.int64, device="cuda")
            sts = torch.zeros(L.RENUM_NSTATS, dtype=torch.int64, device="cuda")
            ones = torch.full((2,), -1, dtype=torch.int64, device="cuda")

        def issue():
            eng.run_renum_device(L.make_params(n, m), coin, R_, F, o, T, d_decisions=dec.data_ptr(),
                                 d_outcome=out.data_ptr(), d_decided=dcd.data_ptr(),
                                 d_counters=cnt.data_ptr(), d_witness=wit.data_ptr(),
                                 d_stats=sts.data_ptr(), stream=s.cuda_stream)

        def reset():
            with torch.cuda.stream(s):
                dec.fill_(-1)
                out.fill_(255)
                dcd.fill_(77)
                cnt.zero_()
                wit.fill_(-1)
                sts.zero_()
                sts[2:4].copy_(ones)

        def verify(what):
            torch.cuda.synchronize()
            same(dec.cpu().numpy().view(np.uint64), ref[0], f"{what} decisions")
            same(out.cpu().numpy(), ref[1], f"{what} outcome")
            same(dcd.cpu().numpy(), ref[2], f"{what} decided")
            assert dict(zip(L.COUNTER_NAMES, cnt.cpu().tolist())) == ref[3], what
            assert cnt.cpu().tolist()[12:] == [0, 0, 0, 0], what
            w = int(wit.cpu().numpy().view(np.uint64)[0])
            assert (None if w == L.NO_WITNESS else w) == ref[4], what
            assert stats_of(sts) == ref[5], what

        reset()
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


# --- 9. errors ----------------------------------------------------------------------------------
def test_errors(engine):
    from ba_amd import lib as L

    def code(coin=LOCAL, n=4, m=1, R_=1, F=0b0010, o=A, **kw):
        with pytest.raises(L.BAError) as e:
            engine.run_renum(coin, n, m, R_, F, o, **kw)
        return e.value.code

    assert code(first=0, count=4097) == L.EINVAL           # past 2^12
    assert code(first=4096, count=1) == L.EINVAL
    assert code(first=32, count=1) == L.EINVAL             # not a multiple of 64
    assert code(o=3) == L.EINVAL
    assert code(coin=2, count=1) == L.EINVAL
    assert code(R_=0, count=1) == L.EINVAL
    assert code(R_=17, count=1) == L.EINVAL
    assert code(lie_mode=L.LIE_TABLE) == L.ENOTSUP
    assert code(engine=L.ENGINE_FUSED) == L.EINVAL
    assert code(engine=L.ENGINE_LEVELS) == L.EINVAL
    assert code(faulty_mode=L.FAULTY_RANDOM) == L.EINVAL
    assert code(faulty_mode=L.FAULTY_EXACT) == L.EINVAL
    assert code(order_mode=L.ORDER_RANDOM) == L.EINVAL
    assert code(order_mode=L.ORDER_CONST) == L.EINVAL
    assert code(n=0, count=1) == L.EINVAL
    assert code(n=33, count=1) == L.EINVAL
    assert code(m=11, count=1) == L.EINVAL
    assert code(n=17, m=0, F=0, coin=COMMON, count=2) == L.ETOOBIG   # 1 bit, but n > 16
    assert code(n=32, m=0, F=0, count=64) == L.ETOOBIG
    assert code(n=17, m=0, count=64) == L.ETOOBIG                    # 65 bits and n > 16
    assert code(n=5, R_=4, F=0b00100, count=64) == L.ETOOBIG         # 64 bits
    assert code(n=16, F=0b1, count=64) == L.ETOOBIG                  # 75 bits
    # m = 9 and 10 are accepted, as in RAND
    res = engine.run_renum(LOCAL, 4, 10, 1, 0b0010, A, first=0, count=64)
    assert res.counters["trials"] == 64 and res.counters["in_bound"] == 0
    # the device entry returns the same codes
    cnt = L.Counters()

    def dcode(p, coin=LOCAL, R_=1, F=0b0010, o=A, count=16):
        return engine.lib.ba_renum_run_device(engine.handle, ctypes.byref(p), coin, R_, F, o, count, None,
                                              None, None, ctypes.addressof(cnt), None, None, None)

    assert dcode(L.make_params(4, 1), count=4097) == L.EINVAL
    assert dcode(L.make_params(4, 1, first_trial=32), count=1) == L.EINVAL
    assert dcode(L.make_params(4, 1), o=3) == L.EINVAL
    assert dcode(L.make_params(4, 1), coin=2) == L.EINVAL
    assert dcode(L.make_params(4, 1), R_=0) == L.EINVAL
    assert dcode(L.make_params(4, 1), R_=17) == L.EINVAL
    assert dcode(L.make_params(4, 1, lie_mode=L.LIE_TABLE)) == L.ENOTSUP
    assert dcode(L.make_params(4, 1, engine=L.ENGINE_LEVELS)) == L.EINVAL
    assert dcode(L.make_params(4, 1, faulty_mode=L.FAULTY_EXACT)) == L.EINVAL
    assert dcode(L.make_params(4, 1, order_mode=L.ORDER_CONST)) == L.EINVAL
    assert dcode(L.make_params(0, 1)) == L.EINVAL
    assert dcode(L.make_params(33, 1)) == L.EINVAL
    assert dcode(L.make_params(4, 11)) == L.EINVAL
    assert dcode(L.make_params(17, 0), F=0) == L.ETOOBIG
    assert dcode(L.make_params(5, 1), R_=4, F=0b00100) == L.ETOOBIG
    assert engine.lib.ba_renum_run_device(engine.handle, ctypes.byref(L.make_params(4, 1)), LOCAL, 1, 0b0010, A,
                                          16, None, None, None, None, None, None, None) == L.EINVAL  # no d_counters
    assert engine.lib.ba_renum_run_device(None, ctypes.byref(L.make_params(4, 1)), LOCAL, 1, 0b0010, A, 16,
                                          None, None, None, ctypes.addressof(cnt), None, None, None) == L.EINVAL
    # count = 0: BA_OK with zero counters and counts and no witness
    res = engine.run_renum(LOCAL, 4, 1, 1, 0b0010, A, count=0)
    assert all(v == 0 for v in res.counters.values()) and res.witness is None
    assert res.stats == M.new_stats()
    # F = 0 under COMMON: a space of 2^R coin sequences, all deciding in phase 1
    res = full(engine, COMMON, 4, 1, 3, 0, A)
    assert res.counters["trials"] == 8 and res.counters["validity"] == 8 and res.witness is None
    assert list(res.decisions) == [0b010101] * 8 and list(res.decided) == [1] * 8
    assert res.stats["decided_in"][1] == 8 and res.stats["unsafe"] == 0 == res.stats["undecided"]
    check(res, message(COMMON, 4, 1, 3, 0, A), "F = 0")
    # the ctx still works
    check(full(engine, LOCAL, 4, 1, 1, 0b0010, A), message(LOCAL, 4, 1, 1, 0b0010, A), "after the errors")
