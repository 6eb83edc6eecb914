"""CPU tests of the SM(m) enumeration (docs/SEMANTICS.md §12): the two forms of the
reference model (tests/smenum_model.py) against each other, against §12's figures and
against sm_model's coin trials, the library's host-only entries ba_smenum_bits /
ba_smenum_slots against the closed form and the model's slot order, the strategy coding
of ba_amd/lib.py, and the built kernels' registers."""
import re
import subprocess
import tempfile

import numpy as np
import pytest

import ba_oracle as O
import sm_model as SM
import smenum_model as M

A, R = O.ATTACK, O.RETREAT
MSG, COA = M.MESSAGES, M.COALITION

# §12's table: (n, m, F, forms, B per form, violating per form, smallest S per form)
FIGURES = [
    (4, 0, 0b0001, (MSG, COA), (6, 6), (36, 36), (2, 2)),
    (4, 1, 0b0001, (MSG, COA), (6, 6), (0, 0), (None, None)),
    (4, 1, 0b0011, (MSG, COA), (8, 8), (30, 30), (18, 18)),
    (4, 1, 0b0110, (MSG,), (2,), (0,), (None,)),
    (4, 2, 0b0011, (MSG, COA), (8, 8), (0, 0), (None, None)),
    (5, 1, 0b00011, (MSG, COA), (12, 12), (372, 372), (66, 66)),
    (5, 2, 0b00011, (MSG, COA), (12, 12), (0, 0), (None, None)),
    (5, 2, 0b00110, (MSG,), (8,), (0,), (None,)),
    (5, 2, 0b00111, (MSG, COA), (20, 12), (6126, 126), (4098, 258)),
    (5, 3, 0b00111, (MSG, COA), (20, 12), (0, 0), (None, None)),
    (6, 2, 0b000111, (COA,), (18,), (3060,), (4098,)),
    (6, 3, 0b000111, (COA,), (18,), (0,), (None,)),
    (3, 1, 0b011, (MSG, COA), (4, 4), (0, 0), (None, None)),
]


@pytest.mark.parametrize("n,m,F,orders", [(4, 1, 0b0011, (A, R, O.OTHER)), (5, 1, 0b00011, (A,)),
                                          (4, 0, 0b0001, (R,))])
@pytest.mark.parametrize("form", [MSG, COA])
def test_plane_form_equals_chain_form_on_every_strategy(form, n, m, F, orders):
    """Decisions, outcome bytes, all 12 counters and the witness of the whole space."""
    for o in orders:
        sp = M.Space(form, n, m, F, o)
        dec, cnt, wit = sp.run()
        d, out, cnt_c, wit_c = M.run_chain(form, n, m, F, o, 0, sp.size)
        assert cnt == cnt_c and wit == wit_c, (o, cnt, cnt_c, wit, wit_c)
        assert len(cnt) == 12
        assert [sp.trial(dec, S) for S in range(sp.size)] == list(zip(d, out))
        assert wit is not None and cnt["in_bound"] == 0  # all three are beyond f <= m


@pytest.mark.parametrize("n,m,F,forms,bits,viol,first", FIGURES)
def test_figures_of_the_semantics_table(n, m, F, forms, bits, viol, first):
    for form, B, nv, w in zip(forms, bits, viol, first):
        assert M.bits_formula(form, n, m, F) == B
        for o in (A, R):  # both orders give the same counts
            sp = M.Space(form, n, m, F, o)
            assert sp.B == B
            assert sp.violating() == (nv, w), (form, o)
            _, cnt, wit = sp.run()
            inb = bin(F).count("1") <= m
            assert cnt["in_bound"] == (sp.size if inb else 0)
            assert cnt["bound_violations"] == (nv if inb else 0) and wit == w
            assert not (inb and nv), "a violation in bound"


def test_late_release_is_the_smallest_witness_at_4_1():
    """S = 18: the commander shows lieutenant 2 attack; in round 1, the last, traitor 1
    shows lieutenant 2 retreat, which it cannot pass on.  3 attacks, 2 retreats."""
    n, m, F = 4, 1, 0b0011
    assert M.messages_of(MSG, n, m, F, A, 18) == [(0, 0, 2, 1), (1, 1, 2, 0)]
    V = M.vsets_chain(n, m, F, 1, M.messages_of(MSG, n, m, F, A, 18))
    assert V[2] == {0, 1} and V[3] == {1}
    dec, out = M.decide_chain(n, m, F, A, M.messages_of(MSG, n, m, F, A, 18))
    assert dec[1:] == [R, A] and M.violates(out)


@pytest.mark.parametrize("n,m,F", [(5, 2, 0b00111), (5, 3, 0b00111)])
def test_projection_decides_alike_on_a_whole_20_bit_space(n, m, F):
    """Every message-form S and project(S) in the coalition space: the same decision
    planes, so the same decisions and outcome."""
    o = A
    sm, sc = M.Space(MSG, n, m, F, o), M.Space(COA, n, m, F, o)
    assert (sm.B, sc.B) == (20, 12)
    dm, dc = sm.run()[0], sc.run()[0]
    # project() as a table over bits: coalition bit (k, r, v) <- message bits (k, j, r, v)
    src = {}
    for b, (k, j, r, v) in enumerate(sm.slots):
        src.setdefault((k, 0 if k == 0 else M.ANY, r, v), []).append(b)
    table = [src[s] for s in sc.slots]
    for S in (0, 1, 4098, 0xFFFFF, 0x5A5A5, 0x12345):
        P = sum(1 << i for i, bs in enumerate(table) if any((S >> b) & 1 for b in bs))
        assert M.project(n, m, F, o, S) == P
    S = np.arange(sm.size, dtype=np.int64)
    P = np.zeros(sm.size, np.int64)
    for i, bs in enumerate(table):
        P |= (np.bitwise_or.reduce([(S >> b) & 1 for b in bs]) << i)
    bits = lambda x, size: np.unpackbits(  # noqa: E731
        np.frombuffer(x.to_bytes(size // 8, "little"), np.uint8), bitorder="little")
    mismatches = sum(int((bits(dm[r], sm.size) != bits(dc[r], sc.size)[P]).sum()) for r in range(n - 1))
    assert mismatches == 0


def test_dead_messages_change_nothing():
    """(4,2) F={0,1}: me = 2, K = 1.  Four more send attempts in round 2, traitor 1 to
    loyal 2 and 3, either value: one delivers only when a valid chain exists, which
    needs a loyal signature, and then the recipient holds the value already.  All 2^12
    extended strategies decide as their first 8 bits do."""
    n, m, F, o = 4, 2, 0b0011, A
    base = M.slots(MSG, n, m, F, o)
    assert len(base) == 8 and max(s[0] for s in base) == 1
    extra = [(2, 1, r, v) for r in (2, 3) for v in (0, 1)]
    ref = [M.decide_chain(n, m, F, o, M.messages_of(MSG, n, m, F, o, S)) for S in range(256)]
    for X in range(1 << 12):
        sends = M.messages_of(MSG, n, m, F, o, X & 255) + [e for i, e in enumerate(extra) if (X >> (8 + i)) & 1]
        assert M.decide_chain(n, m, F, o, sends) == ref[X & 255], X
    # the attempts are really tried: one delivers exactly when the other loyal lieutenant
    # got the value from the commander and so signed it in round 1 -- chain (0, other, 1)
    hits = 0
    for X in range(256):
        sends = M.messages_of(MSG, n, m, F, o, X)
        V0 = M.vsets_chain(n, m, F, 1, sends)
        for e in extra:
            log = []
            assert M.vsets_chain(n, m, F, 1, sends + [e], log) == V0
            got = [x for x in log if x[0] == 2]
            other = 5 - e[2]
            if (0, 0, other, e[3]) in sends:
                assert got == [e + ((0, other, 1),)], (X, e)
                assert e[3] in V0[e[2]]  # the recipient holds it: the other one relayed it in round 1
                hits += 1
            else:
                assert got == [], (X, e, got)
    assert hits == 256 * 4 // 2


@pytest.mark.parametrize("n,m", [(4, 1), (5, 2)])
def test_library_bits_and_slots_equal_formula_and_model(n, m):
    from ba_amd import lib as L
    for form in (MSG, COA):
        for F in range(1 << n):
            for o in (A, R):
                sl = L.smenum_slots(form, n, m, F, o)
                assert len(sl) == L.smenum_bits(form, n, m, F) == M.bits_formula(form, n, m, F), bin(F)
                assert sl == M.slots(form, n, m, F, o), (form, bin(F), o)
            assert L.smenum_bits(form, n, m, F | 1 << n | 1 << 31) == len(sl)  # masked to n bits
    assert L.SMENUM_ANY == M.ANY and (L.SMENUM_MESSAGES, L.SMENUM_COALITION) == (MSG, COA)


def test_library_bits_bad_arguments_and_large_cases():
    from ba_amd import lib as L
    bad = 0xFFFFFFFF
    assert L.smenum_bits(2, 4, 1, 1) == bad and L.smenum_bits(MSG, 0, 1, 1) == bad
    assert L.smenum_bits(MSG, 33, 1, 1) == bad and L.smenum_bits(COA, 10, 9, 1) == bad
    for form, n, m, F, o in ((2, 4, 1, 1, A), (MSG, 33, 1, 1, A), (MSG, 4, 9, 1, A), (COA, 0, 1, 1, A),
                             (MSG, 4, 1, 1, 3)):
        with pytest.raises(L.BAError) as ei:
            L.smenum_slots(form, n, m, F, o)
        assert ei.value.code == L.EINVAL
    # the figures the issue of this entry quotes
    for form in (MSG, COA):
        assert L.smenum_bits(form, 25, 0, 0b1) == 48
        assert L.smenum_bits(form, 32, 1, 0b10) == 30
        assert L.smenum_bits(form, 32, 0, 0b1) == 62
    assert L.smenum_bits(MSG, 10, 3, 0b0111) == 70 and L.smenum_bits(COA, 10, 3, 0b0111) == 42
    assert L.smenum_bits(COA, 10, 3, 0b1111) == 48
    assert L.smenum_bits(MSG, 32, 8, 0xFFFF) == M.bits_formula(MSG, 32, 8, 0xFFFF) == len(
        M.slots(MSG, 32, 8, 0xFFFF, A))
    assert L.smenum_bits(MSG, 2, 5, 0b01) == 2 and L.smenum_bits(MSG, 1, 5, 0b1) == 0


def test_decode_and_encode_smstrategy_round_trip():
    from ba_amd import lib as L
    for form, n, m, F, o in ((MSG, 4, 1, 0b0011, A), (COA, 4, 1, 0b0011, R), (MSG, 5, 2, 0b00110, R),
                             (MSG, 5, 2, 0b00110, A), (COA, 10, 3, 0b0111, O.OTHER), (MSG, 5, 2, 0b00111, A)):
        B = L.smenum_bits(form, n, m, F)
        for S in (0, 1, (1 << B) - 1, 0x5A5A5A5A5A5A % (1 << B), 0x123456789ABC % (1 << B)):
            d = L.decode_smstrategy(form, n, m, F, o, S)
            assert d == M.messages_of(form, n, m, F, o, S) and d == sorted(d)
            assert len(d) == bin(S).count("1")
            assert L.encode_smstrategy(form, n, m, F, o, d) == S
    assert L.decode_smstrategy(MSG, 4, 1, 0b0011, A, 18) == [(0, 0, 2, 1), (1, 1, 2, 0)]
    assert L.decode_smstrategy(COA, 4, 1, 0b0011, A, 18) == [(0, 0, 2, 1), (1, L.SMENUM_ANY, 2, 0)]
    with pytest.raises(ValueError):
        L.encode_smstrategy(MSG, 4, 1, 0b0011, A, [(1, 2, 3, 0)])  # a loyal sender's message
    with pytest.raises(ValueError):
        L.encode_smstrategy(MSG, 4, 1, 0b0110, A, [(1, 1, 3, 0)])  # a loyal commander signs attack alone
    with pytest.raises(ValueError):
        L.encode_smstrategy(MSG, 4, 2, 0b0011, A, [(2, 1, 2, 0)])  # round 2 > K: dead, not coded


@pytest.mark.parametrize("n,m,F", [(4, 1, 0b0011), (4, 5, 0b0111), (5, 2, 0b00111), (6, 0, 0b000101),
                                   (7, 3, 0b0010110), (7, 3, 0b0000111), (5, 2, 0b00110), (4, 1, 0b0001)])
def test_coin_trial_as_a_strategy_gives_the_loyal_decisions(n, m, F):
    """64 trials of seed 7, both orders: the strategy read off a k_sm coin trial decides,
    at every loyal lieutenant, as sm_model's chain form of that trial does; the coalition
    form's projection too."""
    coins = SM.Coins(7)
    loyal = [r for r in range(1, n) if not (F >> r) & 1]
    for o in (A, R):
        ob = int(o == A)
        for t in range(64):
            want = [SM.choice(v) for v in SM.vsets_chain(n, m, coins, t, F, ob)]
            for form in (MSG, COA):
                S = M.coin_strategy(form, n, m, F, o, 7, t)
                assert S < 1 << M.bits_formula(form, n, m, F)
                got, out = M.decide_chain(n, m, F, o, M.messages_of(form, n, m, F, o, S))
                assert [got[r - 1] for r in loyal] == [want[r - 1] for r in loyal], (o, t, form)
                assert out & 0b11100 == SM.trial_outcome(n, m, F, o, want) & 0b11100


# the padded loyal counts k_smenum is built for, per form
PADS = (8, 16, 24, 32)


def test_k_smenum_kernels_use_no_spill_and_no_scratch():
    """Every k_smenum<FORM, LP> instantiation: no spilled vector register and no scratch
    memory, so the lieutenants' planes are in registers; no static LDS."""
    import codeobj
    res = {k: v for k, v in codeobj.kernel_resources().items() if "k_smenum" in k}
    assert len(res) == 2 * len(PADS), "k_smenum<FORM, LP> instantiations missing in libba_hip.so"
    for form in (MSG, COA):
        for lp in PADS:
            assert any(f"k_smenumILi{form}ELi{lp}E" in k for k in res), (form, lp)
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
            if "k_smenum" in re.search(r"\.name:\s+(\S+)", blk).group(1):
                seen += 1
                assert int(re.search(r"\.private_segment_fixed_size:\s+(\d+)", blk).group(1)) == 0, blk
                assert int(re.search(r"\.group_segment_fixed_size:\s+(\d+)", blk).group(1)) == 0, blk
    assert seen == 2 * len(PADS)
