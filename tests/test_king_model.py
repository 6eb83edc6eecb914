"""CPU tests of Phase King (docs/SEMANTICS.md §9): the reference model
(tests/king_model.py) against the figures the contract was checked with and against
the theorem (n > 4m, f <= m), its two forms against each other, the `settled`
semantics on hand-made cases, the host-only call counts, and the built kernels'
register spills."""
import pytest

import ba_oracle as O
import king_model as K

# (n, m, f, policy, trials, violations, trials with settled == 255): seed 7,
# FAULTY_EXACT, ORDER_RANDOM, trials 0..T-1; a violation is IC1 or IC2 failing
C, S = K.KING_COIN, K.KING_SPLIT
TABLE = [(5, 1, 1, C, 300, 0, 0), (5, 1, 1, S, 300, 0, 0), (5, 1, 2, C, 300, 46, 58),
         (5, 1, 2, S, 300, 147, 133), (4, 1, 1, C, 300, 28, 40), (8, 2, 2, S, 300, 104, 77),
         (9, 2, 2, C, 300, 0, 0), (9, 2, 3, S, 300, 122, 108), (13, 3, 3, C, 200, 0, 0),
         (13, 3, 4, S, 200, 98, 70), (32, 7, 7, C, 64, 0, 0), (32, 7, 7, S, 64, 0, 0),
         (32, 7, 11, S, 64, 39, 29), (3, 5, 1, C, 100, 34, 18)]
THEOREM = [(5, 1, 256), (9, 2, 256), (13, 3, 256), (17, 4, 192), (32, 7, 64)]


def _table_run(n, m, f, policy, T, form="message"):
    return K.run(n, m, policy, seed=7, faulty_mode=O.FAULTY_EXACT, f=f, order_mode=O.ORDER_RANDOM,
                 batch=T, form=form)


def test_coins_are_the_oracle_lie_stream():
    c = K.Coins(0xBA5EED)
    for t in (0, 5, 64, 777, (1 << 38) + 3):
        for q in (0, 1, 2, 17, 18):
            for x in (1, 2, 3, 32, 34, 35, 32 * 31 + 30):
                assert c(t, q, x) == O.lie(0xBA5EED, t, 128 + q, x)


@pytest.mark.parametrize("n,m,f,policy,T,viol,uns", TABLE)
def test_model_reproduces_contract_table(n, m, f, policy, T, viol, uns):
    dec, out, stl, cnt = _table_run(n, m, f, policy, T)
    assert K.violations(out) == viol
    assert K.unsettled(stl) == uns
    assert all(s == K.UNSETTLED or s <= K.phases(n, m) for s in stl)
    assert cnt["trials"] == T and cnt["undefined_decisions"] == 0
    assert cnt["faulty_total"] == f * T
    inb = f <= m and n > 4 * m
    assert cnt["in_bound"] == (T if inb else 0)
    assert cnt["bound_violations"] == (viol if inb else 0)


@pytest.mark.parametrize("n,m,f,policy,T,viol,uns", TABLE)
def test_plane_form_equals_message_form_on_table(n, m, f, policy, T, viol, uns):
    assert _table_run(n, m, f, policy, T, "plane") == _table_run(n, m, f, policy, T)


@pytest.mark.parametrize("policy", [C, S])
@pytest.mark.parametrize("n,m", [(4, 1), (5, 1), (9, 2)])
def test_plane_form_equals_message_form_across_2_38(n, m, policy):
    """192 trials from first_trial = 2^38 - 64: the plane form keys its coin words by
    the trial word (2^32 - 1, then 2^32 and 2^32 + 1 with the upper counter word set),
    the message form by the trial; every general may be faulty."""
    kw = dict(seed=0x5157ED0123456789, faulty_mode=O.FAULTY_RANDOM, f=n, order_mode=O.ORDER_RANDOM,
              first_trial=2**38 - 64, batch=192)
    msg = K.run(n, m, policy, form="message", **kw)
    assert K.run(n, m, policy, form="plane", **kw) == msg
    assert msg[3]["trials"] == 192 and msg[0][:64] != msg[0][64:128] != msg[0][128:]


@pytest.mark.parametrize("policy", [C, S])
@pytest.mark.parametrize("n,m,T", THEOREM)
def test_no_violation_within_the_bound(n, m, T, policy):
    """n > 4m and f <= m (FAULTY_RANDOM draws f in 0..m): IC1 and IC2 always hold, and
    the loyal generals agree from some phase on."""
    kw = dict(seed=11, faulty_mode=O.FAULTY_RANDOM, f=m, order_mode=O.ORDER_RANDOM, batch=T)
    dec, out, stl, cnt = K.run(n, m, policy, **kw)
    assert K.violations(out) == 0 and K.unsettled(stl) == 0
    assert cnt["in_bound"] == T and cnt["bound_violations"] == 0
    assert cnt["agreement"] == T and cnt["validity"] == cnt["validity_applicable"]
    assert K.run(n, m, policy, form="plane", **kw) == (dec, out, stl, cnt)


def test_settled_on_hand_made_cases():
    # no traitor: everybody holds the order after round 0, whatever the order code
    dec, out, stl, cnt = K.run(5, 1, seed=3, faulty=[0, 0, 0], order=[1, 0, 2], batch=3)
    assert stl == [0, 0, 0]
    assert dec == [0b01010101, 0, 0]
    assert [o & 3 for o in out] == [O.Q_ATTACK, O.Q_RETREAT, O.Q_RETREAT]
    # (5, 1), only the commander faulty, SPLIT: lieutenants 1, 3 hold attack and 2, 4
    # retreat after round 0.  Phase 1: every lieutenant counts two attack votes of the
    # other three lieutenants' and its own, plus the commander's r & 1 -- c1 = 3 at odd
    # r (maj attack), 2 at even r (maj retreat); no one is strong (2 * 3 > 5 + 2 fails),
    # and the king is the traitor itself, who shows r & 1 again: still split.  Phase 2:
    # the same tallies, king = loyal lieutenant 1 with maj attack: all attack.
    dec, out, stl, cnt = K.run(5, 1, S, seed=3, faulty=[1, 1, 1], order=[1, 0, 2], batch=3)
    assert stl == [2, 2, 2] and dec == [0b01010101] * 3
    assert cnt["agreement"] == 3 and cnt["validity_applicable"] == 0 and cnt["in_bound"] == 3
    hist = K.history_message(5, 1, S, K.Coins(3), 0, 1, 1)
    assert hist == [[1, 1, 0, 1, 0], [1, 1, 0, 1, 0], [1, 1, 1, 1, 1]]
    # the same under coins: never later than the loyal king's phase
    dec, out, stl, cnt = K.run(5, 1, C, seed=3, faulty=[1] * 64, order=[1, 0] * 32, batch=64)
    assert set(stl) <= {0, 1, 2} and cnt["agreement"] == 64
    # nobody or one general loyal: agreed from round 0 on
    assert K.run(3, 1, C, seed=1, faulty=[0b111, 0b110, 0b011], order=[1, 1, 0], batch=3)[2] == [0, 0, 0]
    # agreement lost again does not count: settled is about every later phase too
    assert K.settled_of(3, 0, [[1, 1, 1], [1, 0, 1], [0, 0, 0], [0, 0, 0]]) == 2
    assert K.settled_of(3, 0, [[1, 1, 1], [1, 0, 1]]) == K.UNSETTLED
    assert K.settled_of(3, 0b010, [[1, 1, 1], [1, 0, 1]]) == 0


def test_coin_calls_and_phases_formulas():
    from ba_amd import lib as L
    for n in range(0, 34):
        for m in range(0, 10):
            ok = 1 <= n <= 32 and m <= 8
            P = min(m, n - 1) + 1 if ok else 0
            want = ((n + 1) // 2) * (1 + P * (n + 1)) if ok else 0
            assert L.king_phases(n, m) == P == K.phases(n, m), (n, m)
            assert L.king_coin_calls(n, m) == want == K.coin_calls(n, m), (n, m)
    assert L.king_coin_calls(10, 3) == 225 and L.king_coin_calls(32, 7) == 4240
    assert L.king_phases(32, 7) == 8 and L.king_phases(3, 5) == 3


def test_k_king_kernels_do_not_spill():
    import codeobj
    res = {k: v for k, v in codeobj.kernel_resources().items() if "k_king" in k}
    assert len(res) >= 4, "k_king<GEN, COIN> instantiations missing in libba_hip.so"
    for name, r in res.items():
        assert r["vgpr_spill"] == 0, (name, r)
    # and no scratch memory at all (the metadata's private segment size)
    import re
    import subprocess
    import tempfile
    seen = 0
    for co in codeobj.code_objects():
        with tempfile.NamedTemporaryFile(suffix=".co") as f:
            f.write(co)
            f.flush()
            notes = subprocess.run([f"{codeobj.LLVM}/llvm-readelf", "--notes", f.name], check=True,
                                   capture_output=True, text=True).stdout
        for blk in notes.split("- .agpr_count")[1:]:
            if "k_king" in re.search(r"\.name:\s+(\S+)", blk).group(1):
                seen += 1
                assert int(re.search(r"\.private_segment_fixed_size:\s+(\d+)", blk).group(1)) == 0, blk
    assert seen == len(res)
