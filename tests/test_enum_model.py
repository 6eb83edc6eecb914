"""CPU tests of the exhaustive traitor-strategy enumeration (docs/SEMANTICS.md §8): the
reference model (tests/enum_model.py), its two forms against each other and against
the pinned whole-space figures, the host-only functions ba_enum_bits / ba_enum_slots,
decode_strategy, and the built kernels' resources."""
import itertools
import re
import subprocess
import tempfile

import pytest

import ba_oracle as O
import enum_model as E

A, R = O.ATTACK, O.RETREAT
ANY = None
# (n, m, F, o): (B, agreement, validity, violations, witness, (quorum retreat, attack,
# undetermined), undefined decisions, attack decisions) over the whole space; None = not pinned
PINNED = {
    (3, 1, 0b010, A): (1, 2, 1, 1, 0, ANY, ANY, ANY),
    (4, 1, 0b0001, A): (3, 8, 0, 0, None, (4, 4, 0), 0, 12),
    (4, 1, 0b0010, A): (2, 4, 4, 0, None, ANY, ANY, ANY),
    (4, 1, 0b0011, A): (4, 12, 0, 4, 5, (6, 6, 4), 0, 20),
    (4, 1, 0b0110, A): (2, 4, 3, 1, 0, ANY, ANY, ANY),
    (4, 1, 0b0110, R): (2, 4, 3, 1, 3, ANY, ANY, ANY),
    (5, 1, 0b00110, A): (4, 10, 9, 7, 0, ANY, ANY, ANY),
    (5, 1, 0b00011, A): (6, 28, 0, 36, 9, (20, 20, 24), 96, 68),
    (6, 1, 0b000111, A): (9, 296, 0, 216, 11, (364, 148, 0), ANY, ANY),
    (4, 2, 0b0110, A): (4, 16, 7, 9, 0, (9, 0, 7), ANY, 7),
    (4, 2, 0b0011, R): (6, 54, 0, 10, 13, (47, 7, 10), ANY, ANY),
    (5, 2, 0b00110, A): (12, 2456, 1872, 2224, 0, (0, 4096, 0), 2560, 13312),
    (5, 2, 0b00110, R): (12, 2456, 1872, 2224, 15, (4096, 0, 0), 2560, 512),
    (5, 2, 0b00011, A): (12, 4096, 0, 0, None, (1280, 1280, 1536), 6144, 4352),
    (7, 2, 0b0000001, A): (6, 64, 0, 0, None, (22, 22, 20), 120, 132),
    (7, 2, 0b0000001, R): (6, 64, 0, 0, None, (22, 22, 20), 120, 132),
}


def _figures(n, m, F, o, form):
    dec, out, cnt, wit = E.run(n, m, F, o, form=form)
    return (dec, out, cnt, wit)


@pytest.mark.parametrize("case", sorted(PINNED))
def test_pinned_whole_space_figures_both_forms(case):
    n, m, F, o = case
    B, agree, valid, viol, wit, q, undef, att = PINNED[case]
    lev = _figures(n, m, F, o, "levels")
    assert lev == _figures(n, m, F, o, "rec")
    _, out, cnt, w = lev
    assert E.bits(n, m, F) == B and cnt["trials"] == 1 << B
    assert (cnt["agreement"], cnt["validity"], E.violations(out)) == (agree, valid, viol)
    assert w == (E.NO_WITNESS if wit is None else wit)
    if q is not ANY:
        assert (cnt["quorum_retreat"], cnt["quorum_attack"], cnt["quorum_undetermined"]) == q
    if undef is not ANY:
        assert cnt["undefined_decisions"] == undef
    if att is not ANY:
        assert cnt["attack_decisions"] == att
    me = O.effective_depth(n, m)
    inb = bin(F).count("1") <= me and n > 3 * me
    assert cnt["in_bound"] == (cnt["trials"] if inb else 0)
    assert cnt["bound_violations"] == (viol if inb else 0)
    assert cnt["faulty_total"] == bin(F).count("1") << B


def test_zero_bit_spaces():
    """No traitor: one strategy, no violation.  Every general a traitor at (4, 1): every
    slot of a faulty sender is dead, still one strategy."""
    _, out, cnt, wit = E.run(4, 1, 0, A)
    assert E.bits(4, 1, 0) == 0 and cnt["trials"] == 1 and wit == E.NO_WITNESS
    assert cnt["agreement"] == cnt["validity"] == 1
    assert E.bits(4, 1, 0b1111) == 0 and E.dead_slots(4, 1, 0b1111) == 9
    assert E.run(4, 1, 0b1111, A)[2]["trials"] == 1


@pytest.mark.parametrize("n,m", [(4, 1), (5, 1), (4, 2), (5, 2)])
def test_both_forms_agree_on_every_small_space(n, m):
    for F, o in itertools.product(range(1 << n), (0, 1, 2)):
        if E.bits(n, m, F) <= 8:
            assert E.run(n, m, F, o) == E.run(n, m, F, o, form="rec"), (F, o)


def test_windows_of_a_large_space_agree():
    """(7, 2) F = {1, 2}: 40 bits; 64 strategies at the top of the space, both forms."""
    first = (1 << 40) - 64
    assert E.run(7, 2, 0b0000110, A, first, 64) == E.run(7, 2, 0b0000110, A, first, 64, form="rec")


def test_dead_slots_do_not_reach_loyal_decisions():
    """§8's argument, checked by brute force: with the dead slots of (5, 2) F = {0, 1, 2}
    set to attack instead of retreat no loyal lieutenant's decision changes."""
    n, m, F = 5, 2, 0b00111
    L, me = n - 1, O.effective_depth(n, m)
    index = {key: i for i, key in enumerate(E.free_slots(n, m, F))}

    def decisions(S, dead_value):
        def level(tau):
            cls = E.slot_class(F, tau)
            if cls == E.TRUTH:
                return 1 if len(tau) == 1 else level(tau[:-1])
            if cls == E.DEAD:
                return dead_value
            return (S >> index[(len(tau) - 1, O.path_rank(tau, L))]) & 1

        def resolve(sigma, r):
            v = level(sigma + (r,))
            if len(sigma) == me:
                return v
            vals = [v] + [resolve(sigma + (j,), r) for j in range(L) if j not in sigma and j != r]
            a, c = sum(vals), len(vals)
            if not sigma:
                return 1 if 2 * a > c else (0 if 2 * a < c else 2)
            return int(2 * a > c)

        return [resolve((), r) for r in range(L) if not (F >> (r + 1)) & 1]

    B = len(index)
    for S in range(0, 1 << B, 7):
        assert decisions(S, 0) == decisions(S, 1), S


def test_symmetry_counters_depend_on_the_class_only():
    ref = E.run(5, 2, 0b00110, A)[2]
    for F in (0b01010, 0b11000):
        assert E.run(5, 2, F, A)[2] == ref


# ---------------------------------------------------------------------------
# the library's host-only functions
# ---------------------------------------------------------------------------
def test_enum_bits_formula_and_model():
    from ba_amd import lib as L
    for n in range(1, 8):
        for m in range(0, 4):
            for F in range(1 << n):
                want = E.bits_formula(n, m, F)
                assert L.enum_bits(n, m, F) == want == E.bits(n, m, F), (n, m, F)
    for (n, m, F), want in {(7, 2, 0b1): 6, (7, 2, 0b10): 25, (7, 2, 0b11): 30, (7, 2, 0b110): 40,
                            (7, 2, 0b111): 44, (10, 3, 0b1): 9, (10, 3, 0b10): 400,
                            (6, 2, 0b11): 20, (10, 1, 0b1110): 18}.items():
        assert L.enum_bits(n, m, F) == want == E.bits_formula(n, m, F), (n, m, F)
    assert L.enum_bits(4, 1, 0xFFFFFFF0 | 0b0010) == 2  # bits at and above n are ignored
    for n, m in ((0, 1), (33, 1), (4, 9)):
        assert L.enum_bits(n, m, 1) == 0xFFFFFFFF


def test_enum_slots_equal_the_models_ordered_list():
    from ba_amd import lib as L
    for n, m in ((2, 1), (3, 1), (4, 1), (5, 1), (4, 2), (5, 2), (5, 3), (6, 2)):
        for F in range(1 << n):
            if E.bits_formula(n, m, F) <= E.MAX_BITS:
                assert L.enum_slots(n, m, F) == E.free_slots(n, m, F), (n, m, F)
    assert L.enum_slots(7, 2, 0b0000110) == E.free_slots(7, 2, 0b0000110)
    assert L.enum_slots(1, 0, 1) == []


def test_caps():
    from ba_amd import lib as L
    assert L.enum_bits(10, 3, 0b10) == 400
    with pytest.raises(L.BAError) as e:
        L.enum_slots(10, 3, 0b10)
    assert e.value.code == L.ETOOBIG
    assert L.load().ba_tree_slots(16, 5) > E.MAX_SLOTS
    with pytest.raises(L.BAError) as e:
        L.enum_slots(16, 5, 1)
    assert e.value.code == L.ETOOBIG
    with pytest.raises(L.BAError) as e:
        L.enum_slots(33, 1, 1)
    assert e.value.code == L.EINVAL
    # cap < B
    lib = L.load()
    import numpy as np
    lv, sl = np.zeros(4, np.uint32), np.zeros(4, np.uint64)
    assert lib.ba_enum_slots(7, 2, 0b1, lv.ctypes.data, sl.ctypes.data, 4) == L.EINVAL
    assert lib.ba_enum_slots(4, 1, 0b1, lv.ctypes.data, sl.ctypes.data, 4) == 3


def test_decode_strategy_reads_a_witness():
    """(4, 1) F = {0, 1}, attack: the model's witness 5 = 0b0101.  Bits 0 and 1 are the
    commander's messages to the loyal lieutenant ranks 1 and 2, bits 2 and 3 those of
    the faulty lieutenant rank 0 to the same two."""
    from ba_amd import lib as L
    n, m, F = 4, 1, 0b0011
    wit = E.run(n, m, F, A)[3]
    assert wit == 5
    d = L.decode_strategy(n, m, F, wit)
    # free slots: the commander to lieutenant ranks 1, 2; lieutenant rank 0 to ranks 1, 2
    assert list(d) == [(1,), (2,), (0, 1), (0, 2)]
    assert d == {(1,): 1, (2,): 0, (0, 1): 1, (0, 2): 0}
    for k, x in E.free_slots(5, 2, 0b00110):
        assert O.path_rank(L.path_of_rank(5, k, x), 4) == x


def test_recorded_three_traitor_witnesses_are_the_models():
    """profiles/r12a_enum_sweep_n7_m2_f3.jsonl: the GPU's witnesses over the whole 2^44 and
    2^45 spaces of (7, 2) with three traitors.  The model over the strategies up to and
    including each gives the same smallest violating strategy."""
    import json
    import os
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                        "r12a_enum_sweep_n7_m2_f3.jsonl")
    rows = [json.loads(line) for line in open(path)]
    assert sorted((r["faulty_mask"], r["order"], r["bits"]) for r in rows) == \
        [(0b0000111, 0, 44), (0b0000111, 1, 44), (0b0001110, 0, 45), (0b0001110, 1, 45)]
    for r in rows:
        assert r["complete"] and r["covered"] == 1 << r["bits"]
        w = r["witness"]
        count = (w + 64) & ~63  # the words up to the witness's
        assert E.run(7, 2, r["faulty_mask"], r["order"], 0, count)[3] == w, r["faulty_mask"]


def test_k_enum_kernels_use_no_spill_and_no_scratch():
    import codeobj
    res = {k: v for k, v in codeobj.kernel_resources().items() if "k_enum" in k}
    assert len(res) == 9, sorted(res)  # me = 0..8
    adv = {k: v for k, v in codeobj.kernel_resources().items() if "k_adv" in k}
    for name, r in res.items():
        assert r["vgpr_spill"] == 0, (name, r)
        # The walk's uniform state (ranks, masks, trip counts of every depth) outnumbers the
        # SGPRs and part of it is parked in VGPR lanes, as in k_adv, whose walk has the same
        # shape: k_enum may park no more than k_adv does at the same depth.
        me = int(re.search(r"k_enumILi(\d)E", name).group(1))
        cap = min(v["sgpr_spill"] for k, v in adv.items() if f"k_advILi{me}E" in k)
        assert r["sgpr_spill"] <= cap, (name, r, cap)
    # the private segment (scratch) of every k_enum, from the same metadata notes
    seen = 0
    for co in codeobj.code_objects():
        with tempfile.NamedTemporaryFile(suffix=".co") as f:
            f.write(co)
            f.flush()
            notes = subprocess.run([f"{codeobj.LLVM}/llvm-readelf", "--notes", f.name], check=True,
                                   capture_output=True, text=True).stdout
        for blk in notes.split("- .agpr_count")[1:]:
            name = re.search(r"\.name:\s+(\S+)", blk).group(1)
            if "k_enum" in name:
                seen += 1
                assert int(re.search(r"\.private_segment_fixed_size:\s+(\d+)", blk).group(1)) == 0, name
    assert seen == 9
