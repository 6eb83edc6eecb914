"""GPU tests of the SM(m) enumeration (docs/SEMANTICS.md §12): k_smenum through the C ABI
against the two forms of the reference model (tests/smenum_model.py) and against the coin
engine k_sm.  Every comparison is exact: decisions, outcome bytes, all 12 run counters
and the witness."""
import ctypes
import functools
import itertools

import numpy as np
import pytest

import ba_oracle as O
import smenum_model as M

pytestmark = pytest.mark.gpu

A, R, OTHER = O.ATTACK, O.RETREAT, O.OTHER
MSG, COA = M.MESSAGES, M.COALITION


# --- references (computed once, shared) ------------------------------------------------
@functools.lru_cache(maxsize=None)
def chain(form, n, m, F, o, first=0, count=None):
    if count is None:
        count = (1 << M.bits_formula(form, n, m, F)) - first
    dec, out, cnt, wit = M.run_chain(form, n, m, F, o, first, count)
    return np.array(dec, np.uint64), np.array(out, np.uint8), cnt, wit


@functools.lru_cache(maxsize=None)
def space(form, n, m, F, o):
    return M.Space(form, n, m, F, o)


@functools.lru_cache(maxsize=None)
def plane(form, n, m, F, o):
    return space(form, n, m, F, o).run()


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


def full(engine, form, n, m, F, o, **kw):
    return engine.run_smenum(form, n, m, F, o, want_decisions=True, want_outcome=True, **kw)


def sets(n, sizes):
    return [sum(1 << g for g in c) for k in sizes for c in itertools.combinations(range(n), k)]


# --- 1. whole spaces against the chain form --------------------------------------------
@pytest.mark.parametrize("o", [A, R, OTHER])
@pytest.mark.parametrize("form,n,m,F,B", [(MSG, 4, 1, 0b0011, 8), (COA, 4, 1, 0b0011, 8), (MSG, 5, 1, 0b00011, 12),
                                          (COA, 5, 2, 0b00111, 12), (MSG, 4, 0, 0b0001, 6),
                                          (MSG, 5, 2, 0b00110, 8), (COA, 4, 2, 0b0011, 8)])
def test_whole_space_equals_chain_form(engine, form, n, m, F, B, o):
    res = full(engine, form, n, m, F, o)
    assert res.counters["trials"] == 1 << B
    check(res, chain(form, n, m, F, o), f"form {form} ({n},{m}) F={F:#b} o={o}")


# --- 2. whole spaces against the plane form --------------------------------------------
@pytest.mark.parametrize("form,n,m,F,B,o", [(MSG, 5, 2, 0b00111, 20, A), (MSG, 5, 2, 0b00111, 20, R),
                                            (COA, 6, 2, 0b000111, 18, A), (COA, 6, 2, 0b000111, 18, OTHER)])
def test_whole_space_equals_plane_form(engine, form, n, m, F, B, o):
    """Counters and witness of the whole space; decisions and outcome bytes of 200
    strategies from a non-zero multiple of 64."""
    sp = space(form, n, m, F, o)
    dec, cnt, wit = plane(form, n, m, F, o)
    assert sp.B == B
    res = engine.run_smenum(form, n, m, F, o)
    assert res.decisions is None and res.outcome is None
    assert {k: res.counters[k] for k in cnt} == cnt and res.witness == wit
    assert wit == 4098 and cnt["agreement"] == sp.size - {20: 6126, 18: 3060}[B]
    first = 64 * 37
    win = full(engine, form, n, m, F, o, first=first, count=200)
    want = [sp.trial(dec, S) for S in range(first, first + 200)]
    same(win.decisions, np.array([w[0] for w in want], np.uint64), "window decisions")
    same(win.outcome, np.array([w[1] for w in want], np.uint8), "window outcome")


# --- 3. in bound: Lamport's theorem by exhaustion ---------------------------------------
@pytest.mark.parametrize("n,m,cases", [(4, 1, 2 * 5), (5, 2, 2 * 16), (4, 5, 2 * 16)])
def test_no_coalition_strategy_breaks_the_bound(engine, n, m, cases):
    """Every F with |F| <= m and B <= 24, both forms, both orders.  (4,5): me = 2 < m, all
    sixteen sets are in bound."""
    from ba_amd import lib as L
    ran = 0
    for form in (MSG, COA):
        for F in sets(n, range(0, min(m, n) + 1)):
            B = L.smenum_bits(form, n, m, F)
            if B > 24:
                continue
            ran += 1
            for o in (A, R):
                res = engine.run_smenum(form, n, m, F, o)
                c = res.counters
                assert c["trials"] == 1 << B and c["in_bound"] == c["trials"], (F, c)  # the zero is not vacuous
                assert c["bound_violations"] == 0 and res.witness is None, (form, F, o, c, res.witness)
                assert c["agreement"] == c["trials"] and c["validity"] == c["validity_applicable"]
                assert c["validity_applicable"] == (0 if F & 1 else c["trials"])
                assert c["faulty_total"] == bin(F).count("1") * c["trials"] and c["undefined_decisions"] == 0
    assert ran == cases


def test_in_bound_case_counts_are_what_the_bit_cap_leaves():
    """The `cases` above: five, sixteen and sixteen sets per form, none above 24 bits."""
    assert len(sets(4, (0, 1))) == 5 and len(sets(5, (0, 1, 2))) == 16 and len(sets(4, range(5))) == 16
    big = [(form, F) for form in (MSG, COA) for F in sets(5, (0, 1, 2)) if M.bits_formula(form, 5, 2, F) > 24]
    assert big == [] and max(M.bits_formula(MSG, 5, 2, F) for F in sets(5, (0, 1, 2))) == 12
    assert max(M.bits_formula(MSG, 4, 5, F) for F in sets(4, range(5))) == 10


# --- 4. beyond the bound: the witness ---------------------------------------------------
@pytest.mark.parametrize("form,n,m,F,wit", [(MSG, 4, 0, 0b0001, 2), (MSG, 4, 1, 0b0011, 18), (COA, 4, 1, 0b0011, 18),
                                            (MSG, 5, 1, 0b00011, 66), (MSG, 5, 2, 0b00111, 4098),
                                            (COA, 5, 2, 0b00111, 258), (COA, 6, 2, 0b000111, 4098)])
def test_witness_is_the_smallest_violating_strategy(engine, form, n, m, F, wit):
    from ba_amd import lib as L
    for o in (A, R):
        _, cnt, w = plane(form, n, m, F, o)
        assert w == wit
        res = engine.run_smenum(form, n, m, F, o)
        assert res.witness == wit
        assert res.counters["agreement"] == cnt["agreement"] < cnt["trials"]
        assert res.counters["in_bound"] == 0 and res.counters["bound_violations"] == 0
        msgs = L.decode_smstrategy(form, n, m, F, o, res.witness)
        assert msgs == M.messages_of(form, n, m, F, o, res.witness)
        assert M.violates(M.decide_chain(n, m, F, o, msgs)[1])
        # re-run as the last element of its word: nothing below it in the word violates
        first = wit & ~63
        one = full(engine, form, n, m, F, o, first=first, count=wit - first + 1)
        assert one.witness == wit and M.violates(int(one.outcome[-1]))


# --- 5. the two forms decide alike ------------------------------------------------------
def test_message_form_equals_coalition_form_at_the_projection(engine):
    """(5,2) F = {0,1,2}: every S of the 20-bit message space against project(S) in the
    12-bit coalition space, decisions and outcome."""
    n, m, F, o = 5, 2, 0b00111, A
    big, small = full(engine, MSG, n, m, F, o), full(engine, COA, n, m, F, o)
    assert len(big.decisions) == 1 << 20 and len(small.decisions) == 1 << 12
    src = {}
    for b, (k, j, r, v) in enumerate(M.slots(MSG, n, m, F, o)):
        src.setdefault((k, 0 if k == 0 else M.ANY, r, v), []).append(b)
    S = np.arange(1 << 20, dtype=np.int64)
    P = np.zeros(1 << 20, np.int64)
    for i, s in enumerate(M.slots(COA, n, m, F, o)):
        P |= np.bitwise_or.reduce([(S >> b) & 1 for b in src[s]]) << i
    for x in (0, 4098, 0xFFFFF, 0x5A5A5):
        assert int(P[x]) == M.project(n, m, F, o, x)
    same(big.decisions, small.decisions[P], "decisions at the projection")
    same(big.outcome, small.outcome[P], "outcome at the projection")


# --- 6. tie to the coin engine ----------------------------------------------------------
TIES = [(5, 2, (0b00001, 0b00011, 0b00110, 0b00111)), (7, 3, (0b0000001, 0b0000011, 0b0000110, 0b0000111)),
        (10, 3, (0b1, 0b11, 0b110, 0b111))]


@pytest.mark.parametrize("n,m,Fs", TIES)
def test_coin_trials_as_strategies_equal_k_sm(engine, n, m, Fs):
    """Each of 64 k_sm coin trials of one seed is one strategy S; k_smenum at S decides as
    k_sm does in that trial: the loyal lieutenants' decision bits and the IC1 / IC2
    flags.  Only (10,3) F = {0,1,2} in the message form (70 bits) is above the cap."""
    from ba_amd import lib as L
    import sm_model
    seed = 0x7E57ED
    coins = sm_model.Coins(seed)
    skipped = ran = 0
    for F in Fs:
        loyal = sum(3 << (2 * (r - 1)) for r in range(1, n) if not (F >> r) & 1)
        for form in (MSG, COA):
            B = L.smenum_bits(form, n, m, F)
            if B > 48:
                skipped += 1
                continue
            for o in (A, R):
                ref = engine.run_sm(n, m, 64, seed=seed, faulty=[F] * 64, order=[o] * 64)
                for t in range(64):
                    S = M.coin_strategy(form, n, m, F, o, seed, t, coins)
                    first = S & ~63
                    got = full(engine, form, n, m, F, o, first=first, count=min(64, 1 << B))
                    i = S - first
                    assert int(got.decisions[i]) & loyal == int(ref.decisions[t]) & loyal, (form, F, o, t)
                    assert int(got.outcome[i]) & 0b11100 == int(ref.outcome[t]) & 0b11100, (form, F, o, t)
                    ran += 1
    assert skipped == (1 if n == 10 else 0) and ran == 64 * 2 * (2 * len(Fs) - skipped)


# --- 7. edges ---------------------------------------------------------------------------
def test_small_and_degenerate_cases(engine):
    from ba_amd import lib as L
    # n = 1: no lieutenant, one strategy
    for F in (0, 1):
        res = full(engine, MSG, 1, 3, F, A)
        check(res, chain(MSG, 1, 3, F, A), f"n=1 F={F}")
        assert res.counters["trials"] == 1 and int(res.decisions[0]) == 0
    # n = 2: me = 0; a faulty commander has two bits for its one lieutenant
    for F in (0b00, 0b01, 0b10, 0b11):
        for o in (A, R, OTHER):
            for form in (MSG, COA):
                check(full(engine, form, 2, 4, F, o), chain(form, 2, 4, F, o), f"n=2 F={F:#b} o={o}")
    assert L.smenum_bits(MSG, 2, 4, 0b01) == 2 and L.smenum_bits(MSG, 2, 4, 0b10) == 0
    # l = 0: every lieutenant faulty; B = 0 whatever the commander is
    for F in (0b1110, 0b1111):
        for o in (A, R):
            res = full(engine, COA, 4, 2, F, o)
            assert res.counters["trials"] == 1
            check(res, chain(COA, 4, 2, F, o), f"l=0 F={F:#b}")
    # F = 0: one strategy, nobody lies
    res = full(engine, MSG, 4, 1, 0, A)
    assert res.counters["trials"] == 1 and res.counters["validity"] == 1 and res.witness is None
    assert int(res.decisions[0]) == 0b010101
    # m = 0 with faulty lieutenants only: K = 0, B = 0
    check(full(engine, MSG, 5, 0, 0b00110, A), chain(MSG, 5, 0, 0b00110, A), "m=0 c=0")
    # K = 0 with c = 1: m = 0, and me > 0 without a faulty lieutenant
    for n, m, F in ((5, 0, 0b00111), (5, 2, 0b00001)):
        for form in (MSG, COA):
            assert L.smenum_bits(form, n, m, F) == 2 * (n - 1 - bin(F >> 1).count("1"))
            check(full(engine, form, n, m, F, R), chain(form, n, m, F, R), f"K=0 ({n},{m}) F={F:#b}")


@pytest.mark.parametrize("first,count", [((1 << 48) - 4096, 4096), ((1 << 48) - 4096, 64 * 5 + 29),
                                         (1 << 38, 64 * 5 + 29)])
def test_high_bit_planes_and_the_64_bit_word_index(engine, first, count):
    """n = 25, m = 0, F = {0}: 48 free bits, so bits up to 41 of the word index are planes;
    24 loyal lieutenants, the LP = 24 kernel."""
    from ba_amd import lib as L
    assert L.smenum_bits(COA, 25, 0, 1) == 48
    for o, form in ((A, MSG), (R, COA)):
        check(full(engine, form, 25, 0, 1, o, first=first, count=count),
              chain(form, 25, 0, 1, o, first, count), f"first={first} o={o}")


def test_thirty_loyal_lieutenants_and_the_padded_top_kernel(engine):
    """n = 32, m = 1, F = {1}: 30 bits, 30 loyal lieutenants (LP = 32); the commander is
    loyal, so nothing the traitor sends matters.  And 10 loyal ones (LP = 16) under a
    faulty commander and one relay round: (12,1) F = {0,1}, 40 bits."""
    from ba_amd import lib as L
    assert L.smenum_bits(MSG, 32, 1, 0b10) == 30
    for o in (A, R):
        first, count = 64 * 1000, 64 * 3 + 7
        check(full(engine, MSG, 32, 1, 0b10, o, first=first, count=count),
              chain(MSG, 32, 1, 0b10, o, first, count), f"n=32 o={o}")
        res = engine.run_smenum(COA, 32, 1, 0b10, o, first=1 << 29, count=(1 << 20) + 77)
        c = res.counters
        assert c["trials"] == (1 << 20) + 77 == c["agreement"] == c["validity"] == c["in_bound"]
        assert c["attack_decisions"] == (31 * c["trials"] if o == A else 0) and res.witness is None
    assert L.smenum_bits(COA, 12, 1, 0b11) == 40
    for first in (0, (1 << 40) - 256, 0x5A5A5A5A40):
        check(full(engine, COA, 12, 1, 0b11, A, first=first, count=256),
              chain(COA, 12, 1, 0b11, A, first, 256), f"n=12 first={first}")


# --- 8. ranges, chunks, the device entry -------------------------------------------------
@pytest.mark.parametrize("form,n,m,F", [(MSG, 5, 1, 0b00011), (COA, 5, 2, 0b00111)])
def test_three_ranges_sum_to_the_whole_call(engine, form, n, m, F):
    """Ends that are neither tile (4,096) nor word (64) aligned; B = 12."""
    T = (1 << 12) - 64 * 3 - 35
    cuts = [0, 64 * 7, 64 * 29, T]
    for o in (A, R):
        whole = engine.run_smenum(form, n, m, F, o, first=0, count=T)
        parts = [engine.run_smenum(form, n, m, F, o, first=a, count=b - a) for a, b in zip(cuts, cuts[1:])]
        assert whole.counters["trials"] == T
        assert whole.counters == {k: sum(p.counters[k] for p in parts) for k in whole.counters}
        wits = [p.witness for p in parts if p.witness is not None]
        assert whole.witness == (min(wits) if wits else None)
        ref = chain(form, n, m, F, o)
        want = M.run_chain(form, n, m, F, o, 0, 0)[2]
        for S in range(T):
            out = int(ref[1][S])
            want["trials"] += 1
            want["agreement"] += (out >> 2) & 1
            want["validity_applicable"] += (out >> 3) & 1
            want["validity"] += (out >> 4) & 1
            want[["quorum_retreat", "quorum_attack", "quorum_undetermined"][out & 3]] += 1
            want["attack_decisions"] += bin(int(ref[0][S])).count("1")
            want["faulty_total"] += bin(F).count("1")
        assert {k: whole.counters[k] for k in O.COUNTERS} == want


HIGH_FIRST = (1 << 41) | (1 << 33) | (64 * 77)  # a multiple of 64 with bits above 2^32


@pytest.mark.parametrize("form,n,m,F,B,first", [(COA, 10, 3, 0b0000000111, 42, 0), (MSG, 7, 3, 0b0000111, 40, 0),
                                                (COA, 10, 3, 0b0000000111, 42, HIGH_FIRST),
                                                (COA, 10, 3, 0b0000001111, 48, 1 << 47)])
def test_persistent_loop_counters_equal_single_pass_shards(engine, form, n, m, F, B, first):
    """2^30 strategies in one call are 262,144 tiles: every wave of the grid (at most
    eight four-wave blocks per CU) takes tile after tile and carries its totals and its
    witness across them.  Thirty-two shards of 2^25 strategies (8,192 tiles, 2,048 blocks:
    one tile per wave on a 256-CU device) sum to the same counters, and the call's
    witness is the smallest of theirs.  Three traitors are in bound at m = 3; four are
    not: there a witness, if any, must lie in the range."""
    from ba_amd import lib as L
    assert L.smenum_bits(form, n, m, F) == B
    T, K = 1 << 30, 32
    whole = engine.run_smenum(form, n, m, F, A, first=first, count=T)
    parts = [engine.run_smenum(form, n, m, F, A, first=first + i * (T // K), count=T // K) for i in range(K)]
    assert whole.counters == {k: sum(p.counters[k] for p in parts) for k in whole.counters}
    wits = [p.witness for p in parts if p.witness is not None]
    assert whole.witness == (min(wits) if wits else None)
    c = whole.counters
    assert c["trials"] == T
    clean = c["agreement"] == T and c["validity"] == c["validity_applicable"]
    assert (whole.witness is None) == clean
    if F == 0b1111:
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
    form, n, m, F, o, first = COA, 10, 3, 0b0000000111, A, 1 << 41
    assert L.smenum_bits(form, n, m, F) == 42
    T, S = (1 << 26) + 4096 + 229, 1 << 24
    s = torch.cuda.current_stream().cuda_stream

    def run(lo, count, dec, out, cnt, wit):
        engine.run_smenum_device(L.make_params(n, m, first_trial=first + lo), form, F, o, count,
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
        mdec, mout, _, _ = chain(form, n, m, F, o, first + lo, count)
        same(dec[lo:lo + count].cpu().numpy().view(np.uint64), mdec, f"decisions at {lo}")
        same(out[lo:lo + count].cpu().numpy(), mout, f"outcome at {lo}")
    c = dict(zip(L.COUNTER_NAMES, cnt.cpu().tolist()))
    clean = c["agreement"] == T and c["validity"] == c["validity_applicable"]
    assert (int(wit.cpu().numpy().view(np.uint64)[0]) == L.NO_WITNESS) == clean


def test_host_chunks_give_identical_outputs(engine, monkeypatch):
    form, n, m, F = MSG, 5, 1, 0b00011
    first, count = 64 * 2, 64 * 9 + 17
    ref = chain(form, n, m, F, A, first, count)
    one = full(engine, form, n, m, F, A, first=first, count=count)
    monkeypatch.setenv("BA_SMENUM_HOST_CHUNK", "128")
    chunked = full(engine, form, n, m, F, A, first=first, count=count)
    only = engine.run_smenum(form, n, m, F, A, first=first, count=count, want_outcome=True)
    monkeypatch.delenv("BA_SMENUM_HOST_CHUNK")
    for res in (one, chunked):
        check(res, ref, "host path")
    assert only.decisions is None and only.counters == one.counters and only.witness == one.witness
    same(only.outcome, ref[1], "outcome alone")


def test_device_entry_accumulates_counters_and_min_accumulates_the_witness(engine):
    import torch
    from ba_amd import lib as L
    form, n, m, F = MSG, 4, 1, 0b0011
    ref = chain(form, n, m, F, R)
    cnt = torch.zeros(16, dtype=torch.int64, device="cuda")
    wit = torch.full((1,), -1, dtype=torch.int64, device="cuda")  # 2^64 - 1
    s = torch.cuda.current_stream().cuda_stream
    for first in (128, 0):  # the second call lowers the witness
        engine.run_smenum_device(L.make_params(n, m, first_trial=first), form, F, R, 128,
                                 d_counters=cnt.data_ptr(), d_witness=wit.data_ptr(), stream=s)
        torch.cuda.synchronize()
        lo = [t for t in range(first, 256) if M.violates(int(ref[1][t]))][0]
        assert int(wit.cpu().numpy().view(np.uint64)[0]) == lo
    assert dict(zip(L.COUNTER_NAMES, cnt.cpu().tolist())) == ref[2]
    assert cnt.cpu().tolist()[12:] == [0, 0, 0, 0]
    assert int(wit.cpu().numpy().view(np.uint64)[0]) == ref[3] == 18


# --- 9. errors --------------------------------------------------------------------------
def test_errors(engine):
    from ba_amd import lib as L

    def code(form=MSG, n=4, m=1, F=0b0011, o=A, **kw):
        with pytest.raises(L.BAError) as e:
            engine.run_smenum(form, n, m, F, o, **kw)
        return e.value.code

    assert code(first=0, count=257) == L.EINVAL            # past 2^8
    assert code(first=256, count=1) == L.EINVAL
    assert code(first=32, count=1) == L.EINVAL             # not a multiple of 64
    assert code(o=3) == L.EINVAL
    assert code(form=2, count=1) == L.EINVAL
    assert code(lie_mode=L.LIE_TABLE) == L.ENOTSUP
    assert code(engine=L.ENGINE_FUSED) == L.EINVAL
    assert code(engine=L.ENGINE_LEVELS) == L.EINVAL
    assert code(faulty_mode=L.FAULTY_RANDOM) == L.EINVAL
    assert code(faulty_mode=L.FAULTY_EXACT) == L.EINVAL
    assert code(order_mode=L.ORDER_RANDOM) == L.EINVAL
    assert code(order_mode=L.ORDER_CONST) == L.EINVAL
    assert code(n=0, count=1) == L.EINVAL
    assert code(n=33, count=1) == L.EINVAL
    assert code(m=9, count=1) == L.EINVAL
    assert code(n=32, m=0, F=0b1, count=64) == L.ETOOBIG             # 62 bits
    assert code(n=10, m=3, F=0b0111, count=64) == L.ETOOBIG          # 70 bits in the message form
    assert code(form=COA, n=12, m=3, F=0b1111, count=64) == L.ETOOBIG   # 64 in the coalition form
    # the coalition form of the same case fits, and so does the first f beyond the bound
    assert engine.run_smenum(COA, 10, 3, 0b0111, A, first=0, count=64).counters["trials"] == 64
    res = engine.run_smenum(COA, 10, 3, 0b1111, A, first=(1 << 48) - 64, count=64)
    assert res.counters["trials"] == 64 and res.counters["in_bound"] == 0
    # the device entry returns the same codes
    cnt = L.Counters()

    def dcode(p, form=MSG, F=0b0011, o=A, count=16):
        return engine.lib.ba_smenum_run_device(engine.handle, ctypes.byref(p), form, F, o, count, None,
                                               None, ctypes.addressof(cnt), None, None)

    assert dcode(L.make_params(4, 1), count=257) == L.EINVAL
    assert dcode(L.make_params(4, 1, first_trial=32), count=1) == L.EINVAL
    assert dcode(L.make_params(4, 1), o=3) == L.EINVAL
    assert dcode(L.make_params(4, 1), form=2) == L.EINVAL
    assert dcode(L.make_params(4, 1, lie_mode=L.LIE_TABLE)) == L.ENOTSUP
    assert dcode(L.make_params(4, 1, engine=L.ENGINE_LEVELS)) == L.EINVAL
    assert dcode(L.make_params(4, 1, faulty_mode=L.FAULTY_EXACT)) == L.EINVAL
    assert dcode(L.make_params(4, 1, order_mode=L.ORDER_CONST)) == L.EINVAL
    assert dcode(L.make_params(0, 1)) == L.EINVAL
    assert dcode(L.make_params(33, 1)) == L.EINVAL
    assert dcode(L.make_params(4, 9)) == L.EINVAL
    assert dcode(L.make_params(32, 0), F=0b1) == L.ETOOBIG
    assert dcode(L.make_params(10, 3), F=0b0111) == L.ETOOBIG
    assert engine.lib.ba_smenum_run_device(engine.handle, ctypes.byref(L.make_params(4, 1)), MSG, 0b0011, A,
                                           16, None, None, None, None, None) == L.EINVAL  # no d_counters
    assert engine.lib.ba_smenum_run_device(None, ctypes.byref(L.make_params(4, 1)), MSG, 0b0011, A, 16,
                                           None, None, ctypes.addressof(cnt), None, None) == L.EINVAL
    # count = 0: BA_OK with zero counters and no witness
    res = engine.run_smenum(MSG, 4, 1, 0b0011, A, count=0)
    assert all(v == 0 for v in res.counters.values()) and res.witness is None
    # the ctx still works
    check(full(engine, MSG, 4, 1, 0b0011, A), chain(MSG, 4, 1, 0b0011, A), "after the errors")


# --- 10. graph capture ------------------------------------------------------------------
def test_device_entry_is_captured_in_a_graph_and_replayed():
    """ba_smenum_run_device copies nothing from the host, so a capturing stream takes it:
    an eager call on a ctx of its own, the same call captured, two replays with counters
    and witness reset; each equals the model."""
    import torch
    from ba_amd import lib as L
    form, n, m, F, o, T = MSG, 4, 1, 0b0011, R, 256
    ref = chain(form, n, m, F, o)
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
            eng.run_smenum_device(L.make_params(n, m), form, F, o, T, d_decisions=dec.data_ptr(),
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
