"""CPU tests of the King enumeration (docs/SEMANTICS.md §11): the two forms of the
reference model (tests/kenum_model.py) against each other and against king_model /
king3_model, the library's host-only entries ba_kenum_bits / ba_kenum_slots against the
closed form and the model's slot order, the strategy coding of ba_amd/lib.py, and the
built kernels' registers."""
import itertools
import re
import subprocess
import tempfile

import pytest

import ba_oracle as O
import kenum_model as M
import king3_model as K3
import king_model as K

A, R = O.ATTACK, O.RETREAT


@pytest.mark.parametrize("proto,n,m,F", [(M.KING, 4, 1, 0b0010), (M.KING3, 3, 1, 0b001)])
def test_plane_form_equals_message_form_on_every_strategy(proto, n, m, F):
    """Decisions, outcome bytes, all counters and the witness of the whole space."""
    sp = M.Space(proto, n, m, F)
    assert sp.B == (9 if proto == M.KING else 16)
    for o in ((A, R, O.OTHER) if proto == M.KING else (A,)):
        pref, cnt, wit = sp.run(o)
        dec, out, cnt_m, wit_m = M.run_message(proto, n, m, F, o, 0, sp.size)
        assert cnt == cnt_m and wit == wit_m, (o, cnt, cnt_m, wit, wit_m)
        assert [sp.trial(pref, o, S) for S in range(sp.size)] == list(zip(dec, out))
        assert wit is not None and cnt["agreement"] < sp.size  # n = 4m / n = 3m: beyond the bound
        assert cnt["in_bound"] == 0 and cnt["bound_violations"] == 0


@pytest.mark.parametrize("proto", [M.KING, M.KING3])
@pytest.mark.parametrize("n,m", [(4, 1), (5, 1)])
def test_library_bits_and_slots_equal_formula_and_model(proto, n, m):
    from ba_amd import lib as L
    for F in range(1 << n):
        sl = L.kenum_slots(proto, n, m, F)
        assert len(sl) == L.kenum_bits(proto, n, m, F) == M.bits_formula(proto, n, m, F), bin(F)
        assert sl == M.slots(proto, n, m, F), bin(F)
        assert L.kenum_bits(proto, n, m, F | 1 << n | 1 << 31) == len(sl)  # masked to n bits


def test_library_bits_bad_arguments_and_large_cases():
    from ba_amd import lib as L
    bad = 0xFFFFFFFF
    assert L.kenum_bits(2, 4, 1, 1) == bad and L.kenum_bits(M.KING, 0, 1, 1) == bad
    assert L.kenum_bits(M.KING, 33, 1, 1) == bad
    assert L.kenum_bits(M.KING, 10, 9, 1) == bad and L.kenum_bits(M.KING3, 10, 9, 1) != bad
    assert L.kenum_bits(M.KING3, 10, 11, 1) == bad
    for proto, n, m, F in ((2, 4, 1, 1), (M.KING, 33, 1, 1), (M.KING, 4, 9, 1)):
        with pytest.raises(L.BAError) as ei:
            L.kenum_slots(proto, n, m, F)
        assert ei.value.code == L.EINVAL
    # the figures the issue of this entry quotes
    assert L.kenum_bits(M.KING3, 7, 1, 0b0000001) == 48
    assert max(L.kenum_bits(M.KING3, n, 1, 1 << g) for n in range(4, 8) for g in range(n)) == 48
    assert L.kenum_bits(M.KING, 9, 2, 0b110000000) == 42
    # bits is not limited to the n <= 16 of the run entries
    assert L.kenum_bits(M.KING, 32, 8, 0xFFFF) == M.bits_formula(M.KING, 32, 8, 0xFFFF)
    assert L.kenum_bits(M.KING3, 32, 10, 0x7) == M.bits_formula(M.KING3, 32, 10, 0x7) == len(
        M.slots(M.KING3, 32, 10, 0x7))


@pytest.mark.parametrize("proto", [M.KING, M.KING3])
def test_split_as_a_strategy_gives_the_split_engines_loyal_decisions(proto):
    """(5,1), every single and double traitor set, both orders: the strategy that codes
    BA_KING_SPLIT (free value bits i & 1, proposals (1, i & 1)) decides as king_model /
    king3_model's SPLIT run does, at every loyal lieutenant.  Faulty generals may differ:
    what two traitors show each other is dead here and r & 1 there."""
    n, m = 5, 1
    KM = K if proto == M.KING else K3
    sets = [sum(1 << g for g in c) for k in (1, 2) for c in itertools.combinations(range(n), k)]
    assert len(sets) == 15
    for F in sets:
        S = M.split_strategy(proto, n, m, F)
        assert S < 1 << M.bits_formula(proto, n, m, F) <= 1 << M.MAX_BITS
        for o in (A, R):
            ob = int(o == A)
            want = KM.history_message(n, m, KM.KING_SPLIT, KM.Coins(0), 0, F, ob)[-1]
            got = M.history_message(proto, n, m, F, ob, M.messages_of(proto, n, m, F, S))[-1]
            loyal = [r for r in range(1, n) if not (F >> r) & 1]
            assert [got[r] for r in loyal] == [want[r] for r in loyal], (bin(F), o)
            if bin(F).count("1") == 1:  # no dead message: every general's preference
                assert got == want, (bin(F), o)


def test_coin_as_a_strategy_gives_the_coin_engines_decisions():
    """One traitor, so no dead message: trial t of a COIN run read as a strategy gives all
    of that trial's final preferences."""
    for proto, KM in ((M.KING, K), (M.KING3, K3)):
        for n, m, F in ((5, 1, 0b00001), (5, 1, 0b00100), (7, 2, 0b0000010)):
            for t in (0, 5, 63):
                S = M.coin_strategy(proto, n, m, F, 7, t)
                want = KM.history_message(n, m, KM.KING_COIN, KM.Coins(7), t, F, 1)[-1]
                assert M.history_message(proto, n, m, F, 1, M.messages_of(proto, n, m, F, S))[-1] == want


def test_withheld_proposal_has_two_codes():
    """(lo, hi) = (0, 0) and (0, 1) are one strategy: same messages, same outcome."""
    proto, n, m, F = M.KING3, 3, 1, 0b001
    sl = M.slots(proto, n, m, F)
    hi = next(b for b, s in enumerate(sl) if s[3] == 1)
    S = 0
    assert M.messages_of(proto, n, m, F, S) == M.messages_of(proto, n, m, F, S | 1 << hi)
    assert M.messages_of(proto, n, m, F, S)[sl[hi][:3]] is None
    assert M.messages_of(proto, n, m, F, 1 << (hi - 1))[sl[hi][:3]] == 0
    assert M.messages_of(proto, n, m, F, 3 << (hi - 1))[sl[hi][:3]] == 1


def test_decode_and_encode_kstrategy_round_trip():
    from ba_amd import lib as L
    for proto, n, m, F in ((M.KING, 4, 1, 0b0010), (M.KING, 5, 1, 0b00011), (M.KING3, 3, 1, 0b001),
                           (M.KING3, 7, 1, 0b0000001)):
        B = L.kenum_bits(proto, n, m, F)
        two = [b for b, s in enumerate(M.slots(proto, n, m, F)) if s[3] == 1]
        for S in (0, 1, (1 << B) - 1, 0x5A5A5A5A5A5A % (1 << B), 0x123456789ABC % (1 << B)):
            d = L.decode_kstrategy(proto, n, m, F, S)
            assert d == M.messages_of(proto, n, m, F, S)
            canon = S  # a withheld proposal is coded (0, 0)
            for b in two:
                if not (S >> (b - 1)) & 1:
                    canon &= ~(1 << b)
            assert L.encode_kstrategy(proto, n, m, F, d) == canon
            assert L.decode_kstrategy(proto, n, m, F, canon) == d
    d = L.decode_kstrategy(M.KING, 4, 1, 0b0010, 5)
    k = next(iter(d))
    with pytest.raises(ValueError):
        L.encode_kstrategy(M.KING, 4, 1, 0b0010, {**d, k: None})  # a one-bit message carries 0 / 1
    with pytest.raises(ValueError):
        L.encode_kstrategy(M.KING, 4, 1, 0b0010, {x: v for x, v in d.items() if x != k})
    with pytest.raises(ValueError):
        L.encode_kstrategy(M.KING, 4, 1, 0b0010, {**d, (1, 0, 1): 0})  # a loyal sender's message


# the shapes tests/test_gpu_kenum.py launches
GPU_SHAPES = [(M.KING, 4), (M.KING, 5), (M.KING, 7), (M.KING3, 3), (M.KING3, 4), (M.KING3, 5),
              (M.KING3, 7)]


def test_k_kenum_kernels_use_no_spill_and_no_scratch():
    """Every k_kenum<PROTO, N> instantiation, N = 1..16: no spilled vector register and
    no scratch memory, so the generals' planes are in registers; no static LDS."""
    import codeobj
    res = {k: v for k, v in codeobj.kernel_resources().items() if "k_kenum" in k}
    assert len(res) == 32, "k_kenum<PROTO, N> instantiations missing in libba_hip.so"
    for proto, n in GPU_SHAPES + [(M.KING, 16), (M.KING3, 16)]:
        assert any(f"k_kenumILi{proto}ELi{n}E" in k for k in res), (proto, n)
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
            if "k_kenum" in re.search(r"\.name:\s+(\S+)", blk).group(1):
                seen += 1
                assert int(re.search(r"\.private_segment_fixed_size:\s+(\d+)", blk).group(1)) == 0, blk
                assert int(re.search(r"\.group_segment_fixed_size:\s+(\d+)", blk).group(1)) == 0, blk
    assert seen == 32
