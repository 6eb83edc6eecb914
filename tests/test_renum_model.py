"""CPU tests of the RAND enumeration (docs/SEMANTICS.md §14): the two forms of the
reference model (tests/renum_model.py) against each other and against rand_model, the
cross-check figures computed from rand_model.phase_step, the library's host-only entries
ba_renum_bits / ba_renum_slots against the closed form and the model's slot order, the
strategy decoding of ba_amd/lib.py, and the built kernels' registers."""
import collections
import re
import subprocess
import tempfile

import numpy as np
import pytest

import ba_oracle as O
import rand_model as RM
import renum_model as M

A, R = O.ATTACK, O.RETREAT
LOCAL, COMMON = M.LOCAL, M.COMMON


def histogram(decided):
    return dict(collections.Counter(decided))


@pytest.mark.parametrize("coin,n,R_,F,B", [(LOCAL, 3, 1, 0b010, 8), (COMMON, 4, 1, 0b0001, 13),
                                           (LOCAL, 4, 1, 0b0010, 12), (COMMON, 3, 2, 0b010, 14)])
def test_plane_form_equals_message_form_on_every_strategy(coin, n, R_, F, B):
    """Decisions, outcome bytes, decided bytes, all counters, the witness and the stats of
    the whole space."""
    sp = M.Space(coin, n, 1, R_, F)
    assert sp.B == B == M.bits_formula(coin, n, 1, R_, F)
    for o in (A, R, O.OTHER) if B <= 12 else (R,):
        x, dpl, cnt, wit, st = sp.run(o)
        dec, out, dcd, cnt_m, wit_m, st_m = M.run_message(coin, n, 1, R_, F, o, 0, sp.size)
        assert cnt == cnt_m and wit == wit_m and st == st_m, (o, cnt, cnt_m, wit, wit_m, st, st_m)
        assert [sp.trial(x, dpl, o, S) for S in range(sp.size)] == list(zip(dec, out, dcd))
        assert st["unsafe"] + st["undecided"] + sum(st["decided_in"]) == sp.size


# the issue's cross-checks, computed from rand_model.phase_step with §14's bit order:
# (coin, n, R, F, order, B, first unsafe S, {decided byte: strategies})
CROSS = [
    (LOCAL, 3, 2, 0b010, A, 16, 15, {1: 520, 2: 792, 254: 3376, 255: 60848}),
    (LOCAL, 3, 2, 0b010, R, 16, 4033, {1: 520, 2: 792, 254: 3376, 255: 60848}),
    (COMMON, 3, 2, 0b010, R, 14, 1985, {1: 164, 2: 232, 254: 1048, 255: 14940}),
    (LOCAL, 4, 1, 0b0001, A, 15, None, {1: 11408, 255: 21360}),
    (COMMON, 4, 1, 0b0001, R, 13, None, {1: 2852, 255: 5340}),
    (LOCAL, 4, 1, 0b0010, A, 12, None, {1: 4096}),
    (LOCAL, 4, 1, 0b0010, R, 12, None, {1: 4096}),
    (LOCAL, 4, 1, 0b0110, A, 14, None, {1: 1788, 255: 14596}),
    (LOCAL, 4, 1, 0b0110, R, 14, None, {1: 1788, 255: 14596}),
]


@pytest.mark.parametrize("coin,n,R_,F,o,B,unsafe,hist", CROSS)
def test_message_form_reproduces_the_cross_checks(coin, n, R_, F, o, B, unsafe, hist):
    assert M.bits_formula(coin, n, 1, R_, F) == B
    dec, out, dcd, cnt, wit, st = M.run_message(coin, n, 1, R_, F, o, 0, 1 << B)
    assert histogram(dcd) == hist
    assert st["unsafe_witness"] == unsafe and st["unsafe"] == hist.get(254, 0)
    assert st["undecided"] == hist.get(255, 0)
    if (coin, n, F) == (LOCAL, 4, 0b0001):
        split = sum(1 for d in dec if len({(d >> (2 * r)) & 1 for r in range(n - 1)}) > 1)
        assert split == 8784  # strategies that leave the loyal lieutenants split


def test_plane_form_reproduces_the_larger_cross_checks():
    # (3,1) R=2 LOCAL F={0} attack: 18 bits
    st = M.Space(LOCAL, 3, 1, 2, 0b001).run(A)[4]
    assert st["unsafe_witness"] == 63
    assert (st["decided_in"][1], st["decided_in"][2], st["unsafe"], st["undecided"]) == (1040, 2880, 4848, 253376)
    # (4,1) R=2 COMMON F={1}: 20 bits, every strategy decides in phase 1
    for o in (A, R):
        x, dpl, cnt, wit, st = M.Space(COMMON, 4, 1, 2, 0b0010).run(o)
        assert st["decided_in"][1] == 1 << 20 and st["unsafe"] == 0 == st["undecided"]
        assert wit is None and cnt["bound_violations"] == 0 and cnt["in_bound"] == 1 << 20


def test_a_rand_trial_as_a_strategy_gives_rand_models_history():
    """One traitor, so no dead message: trial t of a COIN or SPLIT run of rand_model read
    as a strategy gives that trial's whole history and decided byte."""
    for coin in (LOCAL, COMMON):
        for n, m, R_, F in ((4, 1, 3, 0b0001), (4, 1, 3, 0b0100), (5, 1, 2, 0b00010)):
            for t in (0, 5, 63):
                for policy, strat in ((RM.KING_COIN, M.coin_strategy), (RM.KING_SPLIT, M.split_strategy)):
                    S = strat(coin, n, m, R_, F, 7, t)
                    assert S < 1 << M.bits_formula(coin, n, m, R_, F) <= 1 << M.MAX_BITS
                    want = RM.history_message(n, m, R_, policy, coin, RM.Coins(7), t, F, 1)
                    got = M.history_message(coin, n, m, R_, F, 1, M.messages_of(coin, n, m, R_, F, S))
                    assert got == want, (coin, n, F, t, policy)


@pytest.mark.parametrize("coin", [LOCAL, COMMON])
@pytest.mark.parametrize("n", [1, 2, 3, 4, 5, 6])
def test_library_bits_and_slots_equal_formula_and_model(coin, n):
    from ba_amd import lib as L
    for R_ in (1, 2, 16):
        for F in range(1 << n):
            B = L.renum_bits(coin, n, 1, R_, F)
            assert B == M.bits_formula(coin, n, 1, R_, F) == len(M.slots(coin, n, 1, R_, F)), (R_, bin(F))
            assert L.renum_bits(coin, n, 1, R_, F | 1 << n | 1 << 31) == B  # masked to n bits
            if R_ < 16:
                assert L.renum_slots(coin, n, 1, R_, F) == M.slots(coin, n, 1, R_, F), (R_, bin(F))
    assert L.RENUM_TOSS == M.TOSS and L.RENUM_COMMON_COIN == M.COMMON_COIN


def test_library_bits_bad_arguments_and_caps():
    from ba_amd import lib as L
    bad = 0xFFFFFFFF
    assert L.renum_bits(2, 4, 1, 1, 1) == bad and L.renum_bits(LOCAL, 0, 1, 1, 1) == bad
    assert L.renum_bits(LOCAL, 33, 1, 1, 1) == bad and L.renum_bits(LOCAL, 4, 11, 1, 1) == bad
    assert L.renum_bits(LOCAL, 4, 10, 1, 1) != bad
    assert L.renum_bits(LOCAL, 4, 1, 0, 1) == bad and L.renum_bits(LOCAL, 4, 1, 17, 1) == bad
    assert L.RENUM_MAX_PHASES == M.MAX_PHASES == 16 and L.RENUM_NSTATS == 20
    for coin, n, m, R_ in ((2, 4, 1, 1), (LOCAL, 33, 1, 1), (LOCAL, 4, 11, 1), (COMMON, 4, 1, 0), (COMMON, 4, 1, 17)):
        with pytest.raises(L.BAError) as ei:
            L.renum_slots(coin, n, m, R_, 1)
        assert ei.value.code == L.EINVAL
    # a slot list needs room for all B bits and all four arrays
    lib, arr = L.load(), [np.zeros(16, np.uint32) for _ in range(4)]
    ptrs = [a.ctypes.data for a in arr]
    assert L.renum_bits(LOCAL, 4, 1, 1, 0b0010) == 12
    assert lib.ba_renum_slots(LOCAL, 4, 1, 1, 0b0010, *ptrs, 11) == L.EINVAL
    assert lib.ba_renum_slots(LOCAL, 4, 1, 1, 0b0010, ptrs[0], None, ptrs[2], ptrs[3], 16) == L.EINVAL
    assert lib.ba_renum_slots(LOCAL, 4, 1, 1, 0b0010, *ptrs, 16) == 12
    assert lib.ba_renum_slots(LOCAL, 4, 1, 1, 0, *ptrs, 16) == 4  # no traitor: the tosses only
    assert [int(a[3]) for a in arr] == [3, 3, 3, L.RENUM_TOSS]
    # the figures the documents quote
    assert L.renum_bits(LOCAL, 5, 1, 3, 0b00100) == 48 and L.renum_bits(LOCAL, 4, 1, 3, 0b0001) == 39
    assert L.renum_bits(COMMON, 4, 1, 3, 0b0001) == 33 and L.renum_bits(COMMON, 4, 1, 4, 0b0010) == 40
    assert L.renum_bits(COMMON, 5, 1, 3, 0b00010) == 39 and L.renum_bits(LOCAL, 7, 2, 1, 0b0000110) == 35
    # one traitor at n = 17 is already past the 48-bit cap: the n cap loses only F = 0
    assert min(L.renum_bits(c, 17, 0, 1, 1 << g) for c in (LOCAL, COMMON) for g in range(17)) == 49
    assert L.renum_bits(COMMON, 32, 0, 16, 0) == 16
    # bits is not limited to the n <= 16 of the run entries
    assert L.renum_bits(LOCAL, 32, 10, 16, 0x7) == M.bits_formula(LOCAL, 32, 10, 16, 0x7)


def test_withheld_proposal_has_two_codes_and_tosses_decode():
    coin, n, m, R_, F = LOCAL, 3, 1, 1, 0b010
    sl = M.slots(coin, n, m, R_, F)
    assert sl == [(1, 1, 0, 0), (1, 1, 2, 0), (2, 1, 0, 0), (2, 1, 0, 1), (2, 1, 2, 0), (2, 1, 2, 1),
                  (3, 0, 0, 2), (3, 2, 2, 2)]
    hi = 3
    assert M.messages_of(coin, n, m, R_, F, 0) == M.messages_of(coin, n, m, R_, F, 1 << hi)
    assert M.messages_of(coin, n, m, R_, F, 0)["messages"][(2, 1, 0)] is None
    assert M.messages_of(coin, n, m, R_, F, 1 << (hi - 1))["messages"][(2, 1, 0)] == 0
    assert M.messages_of(coin, n, m, R_, F, 3 << (hi - 1))["messages"][(2, 1, 0)] == 1
    assert M.messages_of(coin, n, m, R_, F, 1 << 7)["coins"] == {(1, 0): 0, (1, 2): 1}
    assert M.messages_of(COMMON, n, m, 2, F, 1 << 13)["coins"] == {(1, None): 0, (2, None): 1}


def test_decode_rstrategy_equals_the_models():
    from ba_amd import lib as L
    for coin, n, m, R_, F in ((LOCAL, 3, 1, 2, 0b010), (COMMON, 3, 1, 2, 0b001), (LOCAL, 4, 1, 1, 0b0110),
                              (COMMON, 7, 2, 1, 0b0000110), (LOCAL, 5, 1, 3, 0b00100), (COMMON, 4, 1, 2, 0)):
        B = L.renum_bits(coin, n, m, R_, F)
        for S in (0, 1, (1 << B) - 1, 0x5A5A5A5A5A5A % (1 << B), 0x123456789ABC % (1 << B)):
            assert L.decode_rstrategy(coin, n, m, R_, F, S) == M.messages_of(coin, n, m, R_, F, S)


def test_renum_stats_dict():
    from ba_amd import lib as L
    none = L.NO_WITNESS
    st = L.renum_stats([3, 4, 17, none] + list(range(1, 17)))
    assert st == {"unsafe": 3, "undecided": 4, "unsafe_witness": 17, "undecided_witness": None,
                  "decided_in": [0] + list(range(1, 17))}


def test_k_renum_kernels_use_no_spill_and_no_scratch():
    """Every k_renum<COMMON, N> instantiation, N = 1..16 under both coins: no spilled
    vector register and no scratch memory, so the generals' planes x, D and V are in
    registers; no static LDS."""
    import codeobj
    res = {k: v for k, v in codeobj.kernel_resources().items() if "k_renum" in k}
    assert len(res) == 32, "k_renum<COMMON, N> instantiations missing in libba_hip.so"
    for common in (0, 1):
        for n in range(1, 17):
            assert any(f"k_renumILb{common}ELi{n}E" in k for k in res), (common, n)
    for name, r in res.items():
        assert r["vgpr_spill"] == 0, (name, r)
    seen = 0
    for co in codeobj.code_objects():
        with tempfile.NamedTemporaryFile(suffix=".co") as f:
            f.write(co)
            f.flush()
            notes = subprocess.run([f"{codeobj.LLVM}/llvm-readelf", "--notes", f.name], check=True,
                                   capture_output=True, text=True).stdout
        for blk in notes.split("- .agpr_count")[1:]:
            if "k_renum" in re.search(r"\.name:\s+(\S+)", blk).group(1):
                seen += 1
                assert int(re.search(r"\.private_segment_fixed_size:\s+(\d+)", blk).group(1)) == 0, blk
                assert int(re.search(r"\.group_segment_fixed_size:\s+(\d+)", blk).group(1)) == 0, blk
    assert seen == 32
