"""CPU tests of the three-round King algorithm (docs/SEMANTICS.md §10): the reference
model (tests/king3_model.py) against the contract's pinned table and the theorem
(n > 3m, f <= m), its two forms against each other, the worked case preference by
preference, the host-only call counts of the C ABI, and the built kernels' spills
and LDS."""
import re
import subprocess
import tempfile

import pytest

import ba_oracle as O
import king3_model as K3

# (n, m, f, policy, trials, violations, trials with settled == 255): seed 7,
# FAULTY_EXACT, ORDER_RANDOM, trials 0..T-1; a violation is IC1 or IC2 failing.
# The zero rows are the theorem; (6,2) is n = 3m, (3,5) is m > n-1.
C, S = K3.KING_COIN, K3.KING_SPLIT
TABLE = [(4, 1, 1, C, 300, 0, 0), (4, 1, 1, S, 300, 0, 0), (4, 1, 2, C, 300, 71, 68),
         (4, 1, 2, S, 300, 179, 205), (6, 2, 2, S, 300, 66, 66), (7, 2, 2, C, 300, 0, 0),
         (7, 2, 2, S, 300, 0, 0), (7, 2, 3, C, 300, 72, 67), (7, 2, 3, S, 300, 236, 216),
         (10, 3, 3, C, 300, 0, 0), (10, 3, 3, S, 300, 0, 0), (10, 3, 4, S, 300, 226, 205),
         (13, 4, 4, C, 200, 0, 0), (13, 4, 5, S, 200, 153, 133), (32, 10, 10, C, 64, 0, 0),
         (32, 10, 10, S, 64, 0, 0), (32, 10, 11, S, 64, 43, 34), (32, 10, 14, C, 64, 18, 15),
         (3, 5, 1, C, 100, 18, 18), (3, 5, 1, S, 100, 32, 32)]
# the shapes of tests/test_gpu_king3.py
GPU_SHAPES = [(1, 0), (2, 1), (3, 5), (4, 1), (6, 2), (5, 3), (7, 2), (10, 3), (13, 4), (17, 5),
              (31, 10), (32, 10), (32, 0)]


def _table_run(n, m, f, policy, T, form="message"):
    return K3.run(n, m, policy, seed=7, faulty_mode=O.FAULTY_EXACT, f=f, order_mode=O.ORDER_RANDOM,
                  batch=T, form=form)


def test_coins_are_the_oracle_lie_stream_under_tag_192():
    c = K3.Coins(0xBA5EED)
    for t in (0, 5, 64, 777, (1 << 38) + 3):
        for q in (0, 1, 2, 3, 32, 33):
            for x in (1, 2, 3, 32, 34, 35, 32 * 31 + 30):
                assert c(t, q, x) == O.lie(0xBA5EED, t, 192 + q, x)


@pytest.mark.parametrize("n,m,f,policy,T,viol,uns", TABLE)
def test_model_reproduces_contract_table(n, m, f, policy, T, viol, uns):
    dec, out, stl, cnt = _table_run(n, m, f, policy, T)
    assert K3.violations(out) == viol
    assert K3.unsettled(stl) == uns
    assert all(s == K3.UNSETTLED or s <= K3.phases(n, m) for s in stl)
    assert cnt["trials"] == T and cnt["undefined_decisions"] == 0
    assert cnt["faulty_total"] == f * T
    inb = f <= m and n > 3 * m
    assert cnt["in_bound"] == (T if inb else 0)
    assert cnt["bound_violations"] == (viol if inb else 0)
    assert _table_run(n, m, f, policy, T, "plane") == (dec, out, stl, cnt)


@pytest.mark.parametrize("policy", [C, S])
@pytest.mark.parametrize("n,m", GPU_SHAPES)
def test_plane_form_equals_message_form_on_gpu_shapes(n, m, policy):
    """Every general may be faulty; 96 trials from first_trial = 2^38 - 64, so the
    plane form's coin words are keyed with the upper counter word clear, then set."""
    kw = dict(seed=0x5157ED0123456789, faulty_mode=O.FAULTY_RANDOM, f=n, order_mode=O.ORDER_RANDOM,
              first_trial=2**38 - 64, batch=96)
    msg = K3.run(n, m, policy, form="message", **kw)
    assert K3.run(n, m, policy, form="plane", **kw) == msg
    assert msg[3]["trials"] == 96 and msg[3]["undefined_decisions"] == 0


@pytest.mark.parametrize("policy", [C, S])
@pytest.mark.parametrize("n,m,T", [(4, 1, 256), (7, 2, 256), (10, 3, 256), (16, 5, 128), (32, 10, 64)])
def test_no_violation_within_the_bound(n, m, T, policy):
    """n > 3m and f <= m (FAULTY_RANDOM draws f in 0..m): IC1 and IC2 always hold, and
    the loyal generals agree from some phase on."""
    dec, out, stl, cnt = K3.run(n, m, policy, seed=11, faulty_mode=O.FAULTY_RANDOM, f=m,
                                order_mode=O.ORDER_RANDOM, batch=T)
    assert K3.violations(out) == 0 and K3.unsettled(stl) == 0
    assert cnt["in_bound"] == T and cnt["bound_violations"] == 0
    assert cnt["agreement"] == T and cnt["validity"] == cnt["validity_applicable"]


def test_worked_case_preference_by_preference():
    """§10's worked case: (4,1), only the commander faulty, SPLIT, order retreat."""
    for form_hist in (
            K3.history_message(4, 1, S, K3.Coins(3), 0, 1, 0),
            [[pl & 1 for pl in ph] for ph in K3.history_plane_word(4, 1, S, K3.Coins(3), 0, [1], [0])]):
        assert form_hist == [[0, 1, 0, 1], [1, 1, 0, 1], [1, 1, 1, 1]]
    dec, out, stl, cnt = K3.run(4, 1, S, seed=3, faulty=[1], order=[O.RETREAT], batch=1)
    assert stl == [2] and dec == [0b010101]
    assert cnt["agreement"] == 1 and cnt["validity_applicable"] == 0 and cnt["in_bound"] == 1
    # no traitor: everybody holds the order after round 0, whatever the order code
    dec, out, stl, cnt = K3.run(4, 1, seed=3, faulty=[0, 0, 0], order=[1, 0, 2], batch=3)
    assert stl == [0, 0, 0] and dec == [0b010101, 0, 0]
    assert [o & 3 for o in out] == [O.Q_ATTACK, O.Q_RETREAT, O.Q_RETREAT]


def test_retreat_wins_when_both_proposals_hold():
    """n <= 2m: c0 >= n-m and c1 >= n-m can both hold; the proposal is then retreat.
    (5,3), only the commander faulty, SPLIT, order attack: after round 0 the
    preferences are (1,1,0,1,0).  n - m = 2, and every general counts at least two
    retreat votes (c1 = 3 or 2), so all propose retreat although c1 >= 2 as well;
    d0 >= 4 > m everywhere: all retreat after phase 1.  Attack precedence would
    give all attack."""
    hist = K3.history_message(5, 3, S, K3.Coins(0), 0, 1, 1)
    word = K3.history_plane_word(5, 3, S, K3.Coins(0), 0, [1], [1])
    assert hist == [[pl & 1 for pl in ph] for ph in word]
    assert hist[0] == [1, 1, 0, 1, 0]
    assert all(ph == [0, 0, 0, 0, 0] for ph in hist[1:]) and len(hist) == 5


def test_coin_calls_and_phases_formulas():
    from ba_amd import lib as L
    assert [L.king3_phases(*s) for s in ((10, 3), (32, 10), (3, 5), (1, 0))] == [4, 11, 3, 1]
    assert [L.king3_coin_calls(*s) for s in ((10, 3), (32, 7), (32, 10))] == [425, 8336, 11456]
    for n, m in ((0, 1), (33, 1), (10, 11)):
        assert L.king3_phases(n, m) == 0 and L.king3_coin_calls(n, m) == 0
    for n in range(0, 34):
        for m in range(0, 13):
            ok = 1 <= n <= 32 and m <= 10
            P = min(m, n - 1) + 1 if ok else 0
            want = ((n + 1) // 2) * (1 + P * (2 * n + 1)) if ok else 0
            assert L.king3_phases(n, m) == P == K3.phases(n, m), (n, m)
            assert L.king3_coin_calls(n, m) == want == K3.coin_calls(n, m), (n, m)
    # Phase King's own limit stays at 8
    assert L.king_phases(32, 9) == 0 and L.king_phases(32, 8) == 9


def test_k_king3_kernels_do_not_spill_and_lds_fits_four_waves():
    """The four k_king3<GEN, COIN> instantiations: no spilled vector register, no
    scratch memory, and per block the LDS of four waves' images (3,608 B each)."""
    import codeobj
    res = {k: v for k, v in codeobj.kernel_resources().items() if "k_king3" in k}
    assert len(res) == 4, "k_king3<GEN, COIN> instantiations missing in libba_hip.so"
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
            if "k_king3" in re.search(r"\.name:\s+(\S+)", blk).group(1):
                seen += 1
                assert int(re.search(r"\.private_segment_fixed_size:\s+(\d+)", blk).group(1)) == 0, blk
                lds = int(re.search(r"\.group_segment_fixed_size:\s+(\d+)", blk).group(1))
                # F, pref, pa, pr (32 planes each), part (5 x 64), kx, agr[2]
                assert lds == 4 * 8 * (4 * 32 + 5 * 64 + 3), blk
    assert seen == 4
