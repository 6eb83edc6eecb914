"""GPU tests of the exhaustive traitor-strategy enumeration (docs/SEMANTICS.md §8): k_enum
through the C ABI against the level-array reference model (tests/enum_model.py).  Every
comparison is exact: decisions, outcome bytes, all 12 run counters and the witness."""
import ctypes
import functools
import itertools

import numpy as np
import pytest

import ba_oracle as O
import enum_model as E
from test_enum_model import PINNED

pytestmark = pytest.mark.gpu

A, R = O.ATTACK, O.RETREAT
HIGH = 0xFFFFFFFF


@functools.lru_cache(maxsize=None)
def model(n, m, F, o, first=0, count=None):
    """Reference results of a range of strategies (computed once, shared)."""
    dec, out, cnt, wit = E.run(n, m, F, o, first, count)
    return np.array(dec, np.uint64), np.array(out, np.uint8), cnt, wit


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
    assert res.witness == (None if wit == E.NO_WITNESS else wit), what


def full(engine, n, m, F, o, **kw):
    return engine.run_enum(n, m, F, o, want_decisions=True, want_outcome=True, **kw)


@pytest.mark.parametrize("case", sorted(PINNED))
def test_pinned_rows_whole_space(engine, case):
    n, m, F, o = case
    res = full(engine, n, m, F, o)
    check(res, model(n, m, F, o), str(case))
    B, agree, valid, viol, wit = PINNED[case][:5]
    assert res.counters["trials"] == 1 << B
    assert (res.counters["agreement"], res.counters["validity"]) == (agree, valid)
    assert E.violations(res.outcome) == viol and res.witness == wit


@pytest.mark.parametrize("o", [0, 1, 2])
@pytest.mark.parametrize("n,m", [(4, 1), (5, 1), (5, 2), (4, 2)])
def test_every_small_space(engine, n, m, o):
    """Every faulty set with B <= 12: partial words (B < 6), B = 6, several words, dead
    slots (two and more traitors), B = 0."""
    seen = set()
    for F in range(1 << n):
        B = E.bits_formula(n, m, F)
        if B > 12:
            continue
        seen.add(B)
        check(full(engine, n, m, F, o), model(n, m, F, o), f"n={n} m={m} F={F:#b} o={o}")
    want = {(4, 1): {0, 2, 3, 4}, (5, 1): {0, 3, 4, 6}, (4, 2): {0, 3, 4, 5, 6}, (5, 2): {0, 4, 9, 10, 12}}
    assert seen == want[(n, m)]


def test_mask_bits_at_and_above_n_are_ignored(engine):
    for n, m, F, o in ((4, 1, 0b0011, A), (5, 2, 0b00110, R), (5, 1, 0b00011, 2)):
        for high in (HIGH & ~((1 << n) - 1), 1 << n, 1 << 31):
            check(full(engine, n, m, F | high, o), model(n, m, F, o), f"n={n} F={F:#b}|{high:#x}")


@pytest.mark.parametrize("F,first", [(0b0000110, 0), (0b0000110, 1 << 39), (0b0000110, (1 << 40) - 4096),
                                     (0b0000011, 0), (0b0000011, (1 << 30) - 4096)])
def test_high_bit_planes_and_the_64_bit_word_index(engine, F, first):
    """(7, 2): 40 and 30 free bits; windows of 4,096 strategies (one wave's tile) at the
    bottom, the middle and the top of the space."""
    assert E.bits_formula(7, 2, F) == (40 if F == 0b0000110 else 30)
    for o in (A, R):
        check(full(engine, 7, 2, F, o, first=first, count=4096), model(7, 2, F, o, first, 4096),
              f"F={F:#b} first={first} o={o}")


@pytest.mark.parametrize("o", [A, R])
def test_theorem_by_exhaustion_one_faulty_lieutenant_of_seven(engine, o):
    """(7, 2) F = {1}: all 2^25 strategies of one traitorous lieutenant, counters only.
    Within the bound no choice of messages breaks IC1 or IC2."""
    res = engine.run_enum(7, 2, 0b0000010, o)
    c = res.counters
    T = 1 << 25
    assert res.decisions is None and res.outcome is None
    assert c["trials"] == T and c["in_bound"] == T and c["bound_violations"] == 0
    assert c["validity_applicable"] == T and c["validity"] == T and c["agreement"] == T
    assert res.witness is None
    assert c["faulty_total"] == T and c["undefined_decisions"] == 0
    assert c["quorum_attack" if o == A else "quorum_retreat"] == T


def enum_units(count, want_out):
    """Reporting waves of launch_enum (ba_enum.hip): a wave per tile of 64 words (4,096
    strategies); one-wave blocks with per-trial outputs, four-wave blocks without."""
    tiles = ((count + 63) // 64 + 63) // 64
    return tiles if want_out else 4 * ((tiles + 3) // 4)


def test_sink_path_bit_exact(engine):
    """The counter sink of k_enum against the model.  A wave takes 4,096 strategies, so
    a whole space of 16 bits -- one faulty lieutenant of six at m = 2 -- is 16 waves,
    which add straight into the caller's counters; the sink's replicas need more than
    64 waves, i.e. more than 2^18 strategies: the first 67 tiles of the 20-bit space
    of (6, 2) with a faulty commander and lieutenant, with per-trial outputs (67
    one-wave blocks) and without (17 four-wave blocks, 68 waves), then through the
    device entry twice (the first launch must leave the replicas zero)."""
    import torch
    from ba_amd import lib as L
    assert E.bits_formula(6, 2, 0b000010) == 16 and enum_units(1 << 16, True) == 16
    check(full(engine, 6, 2, 0b000010, A), model(6, 2, 0b000010, A), "(6,2) F={1}, whole space")
    F, count = 0b000011, 67 * 4096
    assert E.bits_formula(6, 2, F) == 20
    assert enum_units(count, True) == 67 and enum_units(count, False) == 68
    ref = model(6, 2, F, A, 0, count)
    check(full(engine, 6, 2, F, A, first=0, count=count), ref, "67 tiles, outputs")
    res = engine.run_enum(6, 2, F, A, first=0, count=count)
    assert res.counters == ref[2] and res.witness == (None if ref[3] == E.NO_WITNESS else ref[3])
    cnt = torch.zeros(16, dtype=torch.int64, device="cuda")
    wit = torch.full((1,), -1, dtype=torch.int64, device="cuda")  # 2^64 - 1
    s = torch.cuda.current_stream().cuda_stream
    for _ in range(2):
        engine.run_enum_device(L.make_params(6, 2), F, A, count, d_counters=cnt.data_ptr(),
                               d_witness=wit.data_ptr(), stream=s)
    torch.cuda.synchronize()
    got = cnt.cpu().tolist()
    assert dict(zip(L.COUNTER_NAMES, got)) == {k: 2 * v for k, v in ref[2].items()}
    assert got[12:] == [0, 0, 0, 0]
    assert int(wit.cpu().numpy().view(np.uint64)[0]) == ref[3]


def test_symmetry_counters_depend_on_the_class_only(engine):
    for o in (A, R, 2):
        ref = engine.run_enum(5, 2, 0b00110, o).counters
        assert ref == model(5, 2, 0b00110, o)[2]
        for F in (0b01010, 0b11000):
            assert engine.run_enum(5, 2, F, o).counters == ref


def test_sharding_and_device_accumulation(engine):
    import torch
    from ba_amd import lib as L
    # one call == the sum of 16 shards; its witness == the min of the shards'
    for n, m, F, o, first, count in ((5, 2, 0b00110, R, 0, 1 << 12), (5, 2, 0b00011, A, 0, 1 << 12),
                                     (7, 2, 0b0000011, A, 1 << 24, 1 << 20)):
        whole = engine.run_enum(n, m, F, o, first=first, count=count)
        sh = count // 16
        parts = [engine.run_enum(n, m, F, o, first=first + i * sh, count=sh) for i in range(16)]
        assert whole.counters == {k: sum(p.counters[k] for p in parts) for k in whole.counters}
        wits = [p.witness for p in parts if p.witness is not None]
        assert whole.witness == (min(wits) if wits else None)
        assert whole.counters["trials"] == count
    assert engine.run_enum(5, 2, 0b00110, R).witness == 15
    # every shard of a violating range reports its own lowest violating strategy
    parts = [engine.run_enum(5, 2, 0b00110, A, first=i * 256, count=256) for i in range(16)]
    out = model(5, 2, 0b00110, A)[1]
    for i, p in enumerate(parts):
        bad = [s for s in range(i * 256, (i + 1) * 256) if E.violated(int(out[s]))]
        assert p.witness == (bad[0] if bad else None), i
    # the device entry accumulates the counters and min-accumulates the witness
    ref = model(5, 2, 0b00110, R)
    cnt = torch.zeros(16, dtype=torch.int64, device="cuda")
    wit = torch.full((1,), -1, dtype=torch.int64, device="cuda")  # 2^64 - 1
    s = torch.cuda.current_stream().cuda_stream
    for first in (2048, 0):  # the second call lowers the witness
        engine.run_enum_device(L.make_params(5, 2, first_trial=first), 0b00110, R, 2048,
                               d_counters=cnt.data_ptr(), d_witness=wit.data_ptr(), stream=s)
        torch.cuda.synchronize()
        lo = [t for t in range(first, 4096) if E.violated(int(ref[1][t]))][0]
        assert int(wit.cpu().numpy().view(np.uint64)[0]) == lo
    assert dict(zip(L.COUNTER_NAMES, cnt.cpu().tolist())) == ref[2]
    assert cnt.cpu().tolist()[12:] == [0, 0, 0, 0]
    assert int(wit.cpu().numpy().view(np.uint64)[0]) == ref[3] == 15


@pytest.mark.parametrize("F,o,first", [(0b0000011, A, 0), (0b0000111, A, 1 << 40), (0b0001110, R, 0)])
def test_persistent_loop_counters_equal_single_pass_shards(engine, F, o, first):
    """2^30 strategies in one call are 262,144 tiles: every wave of the grid (at most
    eight four-wave blocks per CU) takes tile after tile and carries its totals and its
    witness across them.  Thirty-two shards of 2^25 strategies (8,192 tiles, 2,048 blocks:
    one tile per wave on a 256-CU device) sum to the same counters, and the call's
    witness is the smallest of theirs.  F = {0,1}: the whole space, in bound; the other
    two: three traitors, violations in most words."""
    T, K = 1 << 30, 32
    whole = engine.run_enum(7, 2, F, o, first=first, count=T)
    parts = [engine.run_enum(7, 2, F, o, first=first + i * (T // K), count=T // K) for i in range(K)]
    assert whole.counters == {k: sum(p.counters[k] for p in parts) for k in whole.counters}
    wits = [p.witness for p in parts if p.witness is not None]
    assert whole.witness == (min(wits) if wits else None)
    assert whole.counters["trials"] == T
    if F == 0b0000011:
        assert whole.witness is None and whole.counters["bound_violations"] == 0
        assert whole.counters["in_bound"] == T and whole.counters["agreement"] == T
    else:
        assert whole.witness == model(7, 2, F, o, first, 4160)[3]  # 4147 + first, 511


def test_persistent_loop_with_outputs_equals_single_pass_shards(engine):
    """With per-trial outputs the blocks are one wave each, at most 32 per CU.  One device
    call of 2^26 + 4,096 + 229 strategies is 16,386 tiles, so blocks take a second and a
    third tile and reuse their decision planes in LDS; the same range as calls of 2^24
    (4,096 tiles each: one tile per block) gives the same bytes, counters and witness, and
    the range's two ends equal the model."""
    import torch
    from ba_amd import lib as L
    n, m, F, o, first = 7, 2, 0b0000111, A, 1 << 41
    T, S = (1 << 26) + 4096 + 229, 1 << 24
    s = torch.cuda.current_stream().cuda_stream

    def run(lo, count, dec, out, cnt, wit):
        engine.run_enum_device(L.make_params(n, m, first_trial=first + lo), F, o, count,
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
        mdec, mout, _, _ = model(n, m, F, o, first + lo, count)
        same(dec[lo:lo + count].cpu().numpy().view(np.uint64), mdec, f"decisions at {lo}")
        same(out[lo:lo + count].cpu().numpy(), mout, f"outcome at {lo}")
    assert int(wit.cpu().numpy().view(np.uint64)[0]) == model(n, m, F, o, first, 8192)[3]


def test_optional_outputs_and_host_chunks(engine, monkeypatch):
    import torch
    from ba_amd import lib as L
    n, m, F, o, first, count = 7, 2, 0b0000011, A, 1 << 12, 4096 + 229
    ref = model(n, m, F, o, first, count)
    s = torch.cuda.current_stream().cuda_stream
    for wd, wo, ww in itertools.product((False, True), repeat=3):
        dec = torch.full((count,), -1, dtype=torch.int64, device="cuda")
        out = torch.full((count,), 255, dtype=torch.uint8, device="cuda")
        cnt = torch.zeros(16, dtype=torch.int64, device="cuda")
        wit = torch.full((1,), -1, dtype=torch.int64, device="cuda")
        engine.run_enum_device(L.make_params(n, m, first_trial=first), F, o, count,
                               d_decisions=dec.data_ptr() if wd else 0,
                               d_outcome=out.data_ptr() if wo else 0, d_counters=cnt.data_ptr(),
                               d_witness=wit.data_ptr() if ww else 0, stream=s)
        torch.cuda.synchronize()
        what = f"dec={wd} out={wo} wit={ww}"
        same(dec.cpu().numpy().view(np.uint64), ref[0] if wd else np.full(count, 2**64 - 1, np.uint64),
             what + " decisions")
        same(out.cpu().numpy(), ref[1] if wo else np.full(count, 255, np.uint8), what + " outcome")
        assert dict(zip(L.COUNTER_NAMES, cnt.cpu().tolist())) == ref[2], what
        assert int(wit.cpu().numpy().view(np.uint64)[0]) == (ref[3] if ww else E.NO_WITNESS), what
    for chunk in (None, "64"):
        if chunk:
            monkeypatch.setenv("BA_ENUM_HOST_CHUNK", chunk)
        for wd, wo in itertools.product((False, True), repeat=2):
            res = engine.run_enum(n, m, F, o, first=first, count=count, want_decisions=wd, want_outcome=wo)
            assert (res.decisions is None) == (not wd) and (res.outcome is None) == (not wo)
            if wd:
                same(res.decisions, ref[0], "host decisions")
            if wo:
                same(res.outcome, ref[1], "host outcome")
            assert res.counters == ref[2]
            assert res.witness == (None if ref[3] == E.NO_WITNESS else ref[3])


def test_decode_strategy_and_rerun_of_the_witness(engine):
    from ba_amd import lib as L
    n, m, F, o = 6, 1, 0b000111, A
    res = engine.run_enum(n, m, F, o)
    assert res.witness == 11
    d = L.decode_strategy(n, m, F, res.witness)
    assert len(d) == L.enum_bits(n, m, F) == 9
    # the commander (faulty) to the loyal lieutenant ranks 2, 3, 4: attack, attack, retreat
    assert [d[(2,)], d[(3,)], d[(4,)]] == [1, 1, 0] and d[(0, 2)] == 1
    assert sum(v << i for i, v in enumerate(d.values())) == res.witness
    for case in ((5, 2, 0b00110, R), (4, 2, 0b0011, R), (5, 1, 0b00011, A)):
        S = engine.run_enum(*case).witness
        first = S & ~63
        one = full(engine, *case, first=first, count=S - first + 1)
        assert E.violated(int(one.outcome[-1]))
        assert one.witness == S  # nothing below S in the window violates
        ref = model(*case)
        assert one.decisions[-1] == ref[0][S] and one.outcome[-1] == ref[1][S]


def test_errors(engine):
    from ba_amd import lib as L

    def code(n=4, m=1, F=0b0011, o=A, **kw):
        with pytest.raises(L.BAError) as e:
            engine.run_enum(n, m, F, o, **kw)
        return e.value.code

    assert code(first=0, count=17) == L.EINVAL           # past 2^4
    assert code(first=64, count=1) == L.EINVAL
    assert code(n=5, m=2, F=0b00110, first=4096, count=1) == L.EINVAL
    assert code(n=5, m=2, F=0b00110, first=32, count=1) == L.EINVAL  # not a multiple of 64
    assert code(o=3) == L.EINVAL
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
    assert code(n=10, m=3, F=0b10, count=64) == L.ETOOBIG   # 400 bits
    assert code(n=16, m=5, F=0b1, count=64) == L.ETOOBIG    # the tree cap
    # the device entry returns the same codes
    cnt = L.Counters()

    def dcode(p, F=0b0011, o=A, count=16):
        return engine.lib.ba_enum_run_device(engine.handle, ctypes.byref(p), F, o, count, None, None,
                                             ctypes.addressof(cnt), None, None)

    assert dcode(L.make_params(4, 1), count=17) == L.EINVAL
    assert dcode(L.make_params(4, 1, first_trial=32), count=1) == L.EINVAL
    assert dcode(L.make_params(4, 1), o=3) == L.EINVAL
    assert dcode(L.make_params(4, 1, lie_mode=L.LIE_TABLE)) == L.ENOTSUP
    assert dcode(L.make_params(4, 1, engine=L.ENGINE_LEVELS)) == L.EINVAL
    assert dcode(L.make_params(4, 1, faulty_mode=L.FAULTY_EXACT)) == L.EINVAL
    assert dcode(L.make_params(4, 1, order_mode=L.ORDER_CONST)) == L.EINVAL
    assert dcode(L.make_params(0, 1)) == L.EINVAL
    assert dcode(L.make_params(33, 1)) == L.EINVAL
    assert dcode(L.make_params(4, 9)) == L.EINVAL
    assert dcode(L.make_params(10, 3), F=0b10) == L.ETOOBIG
    assert dcode(L.make_params(16, 5), F=0b1) == L.ETOOBIG
    assert engine.lib.ba_enum_run_device(engine.handle, ctypes.byref(L.make_params(4, 1)), 0b0011, A, 16,
                                         None, None, None, None, None) == L.EINVAL  # no d_counters
    # count = 0: BA_OK with zero counters and no witness
    res = engine.run_enum(4, 1, 0b0011, A, count=0)
    assert all(v == 0 for v in res.counters.values()) and res.witness is None
    # the ctx still works
    check(full(engine, 4, 1, 0b0011, A), model(4, 1, 0b0011, A), "after the errors")
