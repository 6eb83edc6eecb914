"""The census of the enumeration kernels on live free bits (tests/enum_census.py), checked
against the reference models alone: what tests/test_gpu_enum_census.py feeds the kernels
is within the cap, covers every reachable instantiation, and sits at strategies where the
free bits decide the output.  CPU only; reads tests/golden/enum_census.json, never searches
beyond the two instantiations it regenerates."""
import pytest

import enum_census as C

DOC = C.load()
RECS = DOC["cases"]
KENUM_RENUM = [(f, N) for f in (C.KING, C.KING3, C.LOCAL, C.COMMON) for N in range(1, 17)]
# k_enum<ME>: ME <= n - 2, and the slot map holds sum_k P(n - 1, k + 1) <= 4,096 bytes.
# (7,5) is 1,956 slots; ME = 6 needs n >= 8 (13,699 slots), ME = 7 and 8 need n >= 9.
OM_REACHABLE = [(C.OM, me) for me in range(6)]
OM_UNREACHABLE = [(C.OM, me) for me in (6, 7, 8)]
# Instantiations excluded from a floor BY NAME, with the reason.
FLOOR_EXEMPT = {
    "k_enum<4>": "every case within the cap has F = {0}: B = n - 1 <= 7 < 24",
    "k_enum<5>": "the one shape is (7,5), and within the cap F = {0}: B = 6 < 24",
}


def of(inst):
    return [r for r in RECS if (r["family"], r["sel"]) == inst]


def live(rec):
    return C.shown_live(rec["live"])


def test_unreachable_depths_have_no_case_within_the_limits():
    for inst in OM_UNREACHABLE:
        assert C.candidates(*inst) == []
        n = inst[1] + 2  # the fewest generals with that effective depth
        assert C.tree_slots(n, inst[1]) > C.MAX_SLOTS
    assert sorted(C.reachable()) == sorted(KENUM_RENUM + OM_REACHABLE)


def test_every_case_is_within_the_cap_and_of_its_instantiation():
    seen = set()
    for r in RECS:
        case = C.case_of(r)
        assert C.bits(case) == r["B"] <= C.CAP, r["kernel"]
        assert C.sel_of(case) == r["sel"] and C.kernel_name(r["family"], r["sel"]) == r["kernel"]
        assert case in C.candidates(r["family"], r["sel"]), r["kernel"]
        assert case not in seen
        seen.add(case)
        for S, bs in r["live"]:
            assert 0 <= S < 1 << r["B"] and bs and all(0 <= b < r["B"] for b in bs)
    assert 1 <= min(len(of(i)) for i in KENUM_RENUM + OM_REACHABLE)
    assert max(len(of(i)) for i in KENUM_RENUM + OM_REACHABLE) <= 3


def test_every_recorded_bit_is_live_under_the_model():
    """Two model evaluations per recorded bit (one of them shared per S)."""
    pairs = 0
    for r in RECS:
        case = C.case_of(r)
        for S, bs in r["live"]:
            base = C.evaluate(case, S)
            for b in bs:
                assert C.evaluate(case, S ^ (1 << b)) != base, (r["kernel"], S, b)
                pairs += 1
    assert pairs == sum(len(live(r)) for r in RECS)  # a bit is recorded once per case


def test_fixture_is_what_the_generator_writes():
    """The recorded seed and budgets are the module's, and two instantiations regenerated
    from them equal the file's entries."""
    assert (DOC["seed"], DOC["probe"], DOC["budget"]) == (C.SEED, C.PROBE, C.BUDGET)
    for inst in ((C.KING3, 6), (C.COMMON, 3)):
        assert C.records(*inst, seed=DOC["seed"]) == of(inst), inst


def test_coverage_every_reachable_instantiation_has_a_case():
    for inst in KENUM_RENUM + OM_REACHABLE:
        assert of(inst), C.kernel_name(*inst)
    for inst in OM_UNREACHABLE:
        assert not of(inst)


def test_liveness_floors():
    """N >= 2: a case with at least half of its free bits shown live; N >= 5 (and every
    k_enum depth): such a case with B >= 24.  N = 1 (no lieutenant, B = 0 or toss bits
    that nobody reads) is exempt and has its whole space compared on the GPU."""
    for inst in KENUM_RENUM + OM_REACHABLE:
        family, sel = inst
        name = C.kernel_name(*inst)
        if family != C.OM and sel == 1:
            continue
        half = [r for r in of(inst) if r["B"] and 2 * len(live(r)) >= r["B"]]
        assert half, name
        if (family == C.OM or sel >= 5) and name not in FLOOR_EXEMPT:
            assert any(r["B"] >= 24 for r in half), name
    for name in FLOOR_EXEMPT:  # the exemptions are of cases that cannot exist, not of searches that failed
        inst = (C.OM, int(name[-2]))
        assert C.kernel_name(*inst) == name and max(C.bits(c) for c in C.candidates(*inst)) < 24


@pytest.mark.parametrize("family", [C.KING, C.KING3, C.LOCAL, C.COMMON])
def test_the_three_branches_of_enum_plane_are_live(family):
    """Bits < 6 (constant planes), 6..37 (wlo) and >= 38 (whi): each shown live at N = 16
    and at five or more other N."""
    for what, lo, hi in (("bit < 6", 0, 6), ("bits 6..37", 6, 38), ("bits >= 38", 38, C.CAP)):
        Ns = {r["sel"] for r in RECS if r["family"] == family and any(lo <= b < hi for b in live(r))}
        assert 16 in Ns and len(Ns - {16}) >= 5, (family, what, sorted(Ns))


def test_ranks_and_phases_roles():
    """Where the cap allows a case with >= 2 traitors and >= 2 loyal generals, one is
    recorded with live bits (rf * l + rl with rf > 0 and rl > 0): KING at every N >= 4,
    KING3 and RAND up to N = 10 and 9 (3 * 2 * (N - 2) bits and more per phase above).
    Every RAND instantiation holds a case with R >= 2, with traitors where the cap allows
    (N <= 8)."""
    def nf(x):
        return bin(x["F"] if isinstance(x, dict) else x.F).count("1")

    with_ranks = set()
    for inst in KENUM_RENUM:
        family, N = inst
        cands = C.candidates(*inst)
        if any(nf(c) >= 2 and N - nf(c) >= 2 for c in cands):
            with_ranks.add(inst)
            assert any(nf(r) >= 2 and N - nf(r) >= 2 and 2 * len(live(r)) >= r["B"] for r in of(inst)), \
                C.kernel_name(*inst)
        elif any(nf(c) >= 2 and N - nf(c) >= 1 for c in cands):
            # two traitors beside one loyal general: rf > 0 alone
            assert any(nf(r) >= 2 and live(r) for r in of(inst)), C.kernel_name(*inst)
        if family in C.COIN:
            assert any(r["R"] >= 2 for r in of(inst)), C.kernel_name(*inst)
            if any(c.R >= 2 and nf(c) >= 1 for c in cands):
                assert any(r["R"] >= 2 and nf(r) >= 1 and live(r) for r in of(inst)), C.kernel_name(*inst)
    top = {C.KING: 16, C.KING3: 10, C.LOCAL: 9, C.COMMON: 9}
    assert with_ranks == {(f, N) for f, N in KENUM_RENUM if 4 <= N <= top[f]}


# The cases and windows of test_high_bit_planes_and_the_64_bit_word_index in
# test_gpu_kenum.py, test_gpu_renum.py and test_gpu_enum.py (the 40-bit one).
OLDER_HIGH_BIT_WINDOWS = [
    (C.Case(C.KING3, 7, 1, 0, 0b0000001, None), [((1 << 48) - 4096, 4096), (1 << 38, 64 * 5 + 29)]),
    (C.Case(C.LOCAL, 5, 1, 3, 0b00100, None), [((1 << 48) - 4096, 4096), (1 << 38, 64 * 5 + 29)]),
    (C.Case(C.OM, 7, 2, 0, 0b0000110, None), [(0, 4096), (1 << 39, 4096), ((1 << 40) - 4096, 4096)]),
]


@pytest.mark.parametrize("case,windows", OLDER_HIGH_BIT_WINDOWS)
def test_older_high_bit_windows_are_dead_above_bit_37_and_the_census_is_not(case, windows):
    """Those windows are in bound, so the model's output does not depend on any bit >= 38
    there (every 16th strategy of each window is looked at; the finding is printed).  The
    tests keep what they assert: the 64-bit word index and the ends of the space.  That a
    plane of bits >= 38 is read right is shown by the census cases of the same kernels."""
    B = C.bits(case)
    found = []
    for o in (1, 0):
        c = case._replace(o=o)
        for first, count in windows:
            for S in range(first, first + count, 16):
                base = C.evaluate(c, S)
                found += [(o, S, b) for b in range(38, B) if C.evaluate(c, S ^ (1 << b)) != base]
    print(f"{case.family} ({case.n},{case.m}) F={case.F:#b}: {len(found)} live (S, bit >= 38) pairs in the windows")
    assert not found
    inst = (case.family, C.sel_of(case))
    assert any(b >= 38 for r in of(inst) for b in live(r)), C.kernel_name(*inst)


def test_print_the_census_table():
    """instantiation, role, case, B, live bits by branch, strategies kept (pytest -s)."""
    print()
    print(C.table(DOC))
    total = sum(len(live(r)) for r in RECS)
    print(f"{len(RECS)} cases, {total} live (S, bit) pairs, {sum(len(r['live']) for r in RECS)} strategies")
    assert total > 0
