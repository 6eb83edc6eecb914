"""CPU tests of randomized agreement (docs/SEMANTICS.md §13): the reference model
(tests/rand_model.py), its two forms against each other, the precedence of
`decided`, the phase-1 validity rule, a hand case, safety over every traitor
message and coin outcome, the host-only call count of the C ABI, and the built
kernels' spills and LDS."""
import re
import subprocess
import tempfile

import pytest

import ba_oracle as O
import rand_model as RM

C, S = RM.KING_COIN, RM.KING_SPLIT
LOCAL, COMMON = RM.RAND_LOCAL, RM.RAND_COMMON
# the shapes of tests/test_gpu_rand.py
SHAPES = [(1, 0), (2, 1), (3, 5), (4, 1), (6, 2), (5, 3), (7, 2), (10, 3), (13, 4), (17, 5),
          (31, 10), (32, 10), (32, 0)]


def test_coins_are_the_oracle_lie_stream_under_tag_256():
    c = RM.Coins(0xBA5EED)
    for t in (0, 5, 64, 777, (1 << 38) + 3):
        for q in (0, 1, 2, 3, 191, 192):
            for x in (0, 1, 33, 34, 35, 33 * 31, 32 * 31 + 30):
                assert c(t, q, x) == O.lie(0xBA5EED, t, 256 + q, x)
    # a general's own toss slot is the message slot "i to itself"; the common one is slot 0
    assert [RM.toss_slot(LOCAL, i) for i in (0, 1, 31)] == [0, 33, 32 * 31 + 31]
    assert [RM.toss_slot(COMMON, i) for i in (0, 1, 31)] == [0, 0, 0]


@pytest.mark.parametrize("coin", [LOCAL, COMMON])
@pytest.mark.parametrize("policy", [C, S])
@pytest.mark.parametrize("n,m", SHAPES)
def test_plane_form_equals_message_form(n, m, policy, coin):
    """Every general may be faulty; 96 trials from first_trial = 2^38 - 64, so the
    plane form's coin words are keyed with the upper counter word clear, then set."""
    kw = dict(seed=0x5157ED0123456789, faulty_mode=O.FAULTY_RANDOM, f=n, order_mode=O.ORDER_RANDOM,
              first_trial=2**38 - 64, batch=96)
    msg = RM.run(n, m, 3, policy, coin, form="message", **kw)
    assert RM.run(n, m, 3, policy, coin, form="plane", **kw) == msg
    assert msg[3]["trials"] == 96 and msg[3]["undefined_decisions"] == 0
    assert all(d in (1, 2, 3, RM.UNSAFE, RM.UNDECIDED) for d in msg[2])


def test_decided_precedence():
    """254 beats a phase number, a phase number beats 255; each unsafe condition
    fires alone; D of a faulty general is not waited for."""
    x0 = ([0, 0, 0, 0], [0, 0, 0, 0], [0, 0, 0, 0])
    und = ([1, 1, 1, 1], [0, 1, 1, 1], [0, 1, 1, 1])     # general 0 has not decided
    done = ([1, 1, 1, 1], [1, 1, 1, 1], [1, 1, 1, 1])
    split = ([1, 0, 1, 1], [1, 1, 1, 1], [1, 0, 1, 1])   # two loyal V differ
    moved = ([1, 0, 1, 1], [1, 1, 1, 1], [1, 1, 1, 1])   # x != V
    assert RM.decided_of(4, 0b1000, 1, [x0, und, und]) == RM.UNDECIDED
    assert RM.decided_of(4, 0b0001, 1, [x0, und, und]) == 1   # general 0 is faulty
    assert RM.decided_of(4, 0b1000, 1, [x0, und, done]) == 2
    assert RM.decided_of(4, 0b1000, 1, [x0, done, done]) == 1
    assert RM.decided_of(4, 0b1000, 1, [x0, done, split]) == RM.UNSAFE
    assert RM.decided_of(4, 0b1000, 1, [x0, split, done]) == RM.UNSAFE
    assert RM.decided_of(4, 0b0010, 1, [x0, done, split]) == 1  # the odd one out is faulty
    assert RM.decided_of(4, 0b1000, 1, [x0, und, moved]) == RM.UNSAFE
    assert RM.decided_of(4, 0b0010, 1, [x0, und, moved]) == 2
    # a loyal commander ordered retreat and loyal generals decided attack
    assert RM.decided_of(4, 0b1000, 0, [x0, done]) == RM.UNSAFE
    assert RM.decided_of(4, 0b1001, 0, [x0, done]) == 1       # a faulty commander binds nobody
    # nobody is loyal
    assert RM.decided_of(4, 0b1111, 0, [x0, x0, x0]) == 1


@pytest.mark.parametrize("coin", [LOCAL, COMMON])
@pytest.mark.parametrize("policy", [C, S])
@pytest.mark.parametrize("n,m,T", [(4, 1, 256), (7, 2, 256), (10, 3, 192), (32, 10, 64)])
def test_phase_1_validity_and_safety_within_the_bound(n, m, T, policy, coin):
    """n > 3m and f <= m (FAULTY_RANDOM draws f in 0..m).  A loyal commander: every
    loyal general starts with the order, so all decide it in phase 1 and IC2 holds.
    Any commander: never 254; once decided, IC1 holds."""
    R = 4
    kw = dict(seed=11, faulty_mode=O.FAULTY_RANDOM, f=m, order_mode=O.ORDER_RANDOM, batch=T)
    dec, out, dcd, cnt = RM.run(n, m, R, policy, coin, **kw)
    ins = [RM.K.inputs(n, 11, O.FAULTY_RANDOM, m, O.ORDER_RANDOM, O.ATTACK, t, t, None, None)
           for t in range(T)]
    assert cnt["in_bound"] == T and RM.UNSAFE not in dcd
    seen = 0
    for (fm, oc), o, d in zip(ins, out, dcd):
        if not fm & 1:
            assert d == 1 and (o >> 3) & 1 and (o >> 4) & 1 and (o >> 2) & 1
            seen += 1
        if d != RM.UNDECIDED:
            assert (o >> 2) & 1
    assert seen > T // 2
    assert cnt["bound_violations"] <= sum(1 for d in dcd if d == RM.UNDECIDED)


def test_hand_case_no_traitor_attack():
    """(4,1), no traitor, attack: every general reports attack, c1 = 4 and 2*4 > 5, all
    propose attack, d1 = 4 > 1 and 2*4 > 5: everyone decides attack in phase 1 and no
    coin is tossed."""
    def no_lie(j, i):
        raise AssertionError("nobody is faulty")

    def no_toss(i):
        raise AssertionError("everyone has a value")

    x, D, V = RM.phase_step(4, 1, 0, [1, 1, 1, 1], [0] * 4, [0] * 4, no_lie, no_lie, no_toss)
    assert (x, D, V) == ([1, 1, 1, 1], [1, 1, 1, 1], [1, 1, 1, 1])
    for coin in (LOCAL, COMMON):
        for form_hist in (
                RM.history_message(4, 1, 2, C, coin, RM.Coins(3), 0, 0, 1),
                [tuple([pl & 1 for pl in planes] for planes in ph)
                 for ph in RM.history_plane_word(4, 1, 2, C, coin, RM.Coins(3), 0, [0], [1])]):
            assert [tuple(ph) for ph in form_hist] == [([1] * 4, [0] * 4, [0] * 4)] + 2 * [([1] * 4,) * 3]
        dec, out, dcd, cnt = RM.run(4, 1, 2, C, coin, seed=3, faulty=[0, 0, 0], order=[1, 0, 2], batch=3)
        assert dcd == [1, 1, 1] and dec == [0b010101, 0, 0]
        assert [o & 3 for o in out] == [O.Q_ATTACK, O.Q_RETREAT, O.Q_RETREAT]
        assert cnt["agreement"] == 3 and cnt["validity"] == 3 and cnt["bound_violations"] == 0


def test_a_split_start_needs_the_coin():
    """(4,1), nobody faulty, preferences (1,1,0,0): c1 = 2, nobody proposes, nobody has
    a value, and every general takes its coin."""
    asked = []

    def toss(i):
        asked.append(i)
        return i & 1

    x, D, V = RM.phase_step(4, 1, 0, [1, 1, 0, 0], [0] * 4, [0] * 4, None, None, toss)
    assert asked == [0, 1, 2, 3] and x == [0, 1, 0, 1] and D == [0] * 4


@pytest.mark.parametrize("coin", [LOCAL, COMMON])
@pytest.mark.parametrize("fmask", [0b0010, 0b0001])
def test_exhaustive_safety_in_bound(fmask, coin):
    """(4,1), R = 2, one traitor (a lieutenant; the commander), both orders: over
    every traitor message and every coin outcome no state is unsafe."""
    for ob in (0, 1):
        states = RM.reachable(4, 1, 2, coin, fmask, ob)
        assert not any(s[3] for s in states)
        if fmask & 1:
            assert len(states) > 1
        else:  # a loyal commander: whatever the traitor says, the loyal hold the order
            want = tuple(0 if g == 1 else ob for g in range(4))
            assert states == {(want, (1, 0, 1, 1), want, False)}
        # D set means x = V, and all D-set loyal generals share V
        for x, D, V, _ in states:
            held = {V[g] for g in range(4) if D[g] and not (fmask >> g) & 1}
            assert len(held) <= 1
            assert all(x[g] == V[g] for g in range(4) if D[g] and not (fmask >> g) & 1)


@pytest.mark.parametrize("coin", [LOCAL, COMMON])
def test_exhaustive_check_fires_at_n_equal_3m(coin):
    """(3,1) with F = {1}: n = 3m, and some traitor play is unsafe."""
    assert any(s[3] for ob in (0, 1) for s in RM.reachable(3, 1, 2, coin, 0b010, ob))


def test_coin_calls_formula():
    from ba_amd import lib as L
    assert L.rand_coin_calls(10, 16, L.RAND_COMMON) == 5 * (1 + 2 * 10 * 16) + 16
    assert L.rand_coin_calls(10, 16, L.RAND_LOCAL) == 5 * (1 + 2 * 10 * 16) + 160
    for n in range(0, 34):
        for R in (0, 1, 2, 63, 64, 65):
            for coin in (0, 1, 2):
                ok = 1 <= n <= 32 and 1 <= R <= 64 and coin <= 1
                want = ((n + 1) // 2) * (1 + 2 * n * R) + R * (n if coin == 0 else 1) if ok else 0
                assert L.rand_coin_calls(n, R, coin) == want == RM.coin_calls(n, R, coin), (n, R, coin)
    assert (L.RAND_LOCAL, L.RAND_COMMON, L.RAND_MAX_PHASES, L.RAND_UNDECIDED, L.RAND_UNSAFE) == \
        (RM.RAND_LOCAL, RM.RAND_COMMON, RM.MAX_PHASES, RM.UNDECIDED, RM.UNSAFE)


def test_k_rand_kernels_do_not_spill_and_lds_fits_four_waves():
    """The eight k_rand<GEN, COIN, COMMON> instantiations: no spilled vector register,
    no scratch memory, and per block the LDS of four waves' images (4,648 B each)."""
    import codeobj
    res = {k: v for k, v in codeobj.kernel_resources().items() if "k_rand" in k}
    assert len(res) == 8, "k_rand<GEN, COIN, COMMON> instantiations missing in libba_hip.so"
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
            if "k_rand" in re.search(r"\.name:\s+(\S+)", blk).group(1):
                seen += 1
                assert int(re.search(r"\.private_segment_fixed_size:\s+(\d+)", blk).group(1)) == 0, blk
                lds = int(re.search(r"\.group_segment_fixed_size:\s+(\d+)", blk).group(1))
                # F, pref, pa, pr, D, V (32 planes each), part (5 x 64), chk[5]; fm, oc (64 words each)
                assert lds == 4 * (8 * (6 * 32 + 5 * 64 + 5) + 4 * 2 * 64), blk
    assert seen == 8
