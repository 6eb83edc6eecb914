"""CPU tests of the stalling adversary's reference model (tests/rstall_model.py,
docs/SEMANTICS.md §15): its two forms against each other, the common coin by
exhaustion, the play of a trial as a strategy of §14's space, and the mix of
`decided` classes the GPU comparison rests on."""
import itertools

import pytest

import ba_oracle as O
import rand_model as RM
import renum_model as RN
import rstall_model as SM

SHAPES = [(1, 0), (2, 1), (3, 5), (4, 1), (5, 3), (6, 2), (7, 2), (10, 3), (13, 4), (32, 10)]
SEEDS = [0xBA5EED, 0x5157ED0123456789]
COINS = [SM.RAND_LOCAL, SM.RAND_COMMON]
B = 229  # three full words and a partial one


@pytest.mark.parametrize("R", [1, 3])
@pytest.mark.parametrize("coin", COINS)
@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("n,m", SHAPES)
def test_forms_agree(n, m, seed, coin, R):
    kw = dict(seed=seed, faulty_mode=O.FAULTY_RANDOM, f=n, order_mode=O.ORDER_RANDOM, batch=B)
    msg = SM.run(n, m, R, coin, form="message", **kw)
    pln = SM.run(n, m, R, coin, form="plane", **kw)
    for a, b, what in zip(msg, pln, ("decisions", "outcome", "decided", "counters")):
        assert a == b, what
    assert len(msg[3]) == 12 and msg[3]["trials"] == B


@pytest.mark.parametrize("n,m", [(4, 1), (10, 3)])
@pytest.mark.parametrize("coin", COINS)
def test_forms_agree_over_many_phases(n, m, coin):
    """R = 24: past the phases in which most trials decide, where the GPU tests take the
    plane form as their reference."""
    kw = dict(seed=SEEDS[1], faulty_mode=O.FAULTY_RANDOM, f=n, order_mode=O.ORDER_RANDOM, batch=100)
    assert SM.run(n, m, 24, coin, form="message", **kw) == SM.run(n, m, 24, coin, form="plane", **kw)


@pytest.mark.parametrize("n,m", [(4, 1), (5, 1), (7, 2)])
def test_common_coin_decides_by_phase_two(n, m):
    """Every faulty set with f <= m, both orders, every common-coin sequence of three
    phases: never unsafe, and every loyal general has decided after phase 2."""
    worst = 0
    for f in range(m + 1):
        for bad in itertools.combinations(range(n), f):
            fmask = sum(1 << g for g in bad)
            for ob, seq in itertools.product((0, 1), itertools.product((0, 1), repeat=3)):
                x, D, V = SM.round0(n, fmask, ob), [0] * n, [0] * n
                hist = [(list(x), list(D), list(V))]
                for p in range(3):
                    x, D, V, _, _ = SM.stall_phase(n, m, fmask, x, D, V, lambda i: seq[p])
                    hist.append((list(x), list(D), list(V)))
                dcd = RM.decided_of(n, fmask, ob, hist)
                assert dcd != SM.UNSAFE and dcd <= 2, (fmask, ob, seq, dcd)
                worst = max(worst, dcd)
    assert worst == 2  # a faulty commander does cost a phase


RENUM_CASES = [(coin, fmask) for coin in COINS for fmask in (0b0001, 0b0010)]


@pytest.mark.parametrize("coin,fmask", RENUM_CASES)
def test_a_trial_is_a_strategy_of_renum(coin, fmask):
    """(4,1), R = 3, 16 trials: §14's message form at stall_strategy's S gives the loyal
    generals the states of the STALL message form, and so the same decided byte."""
    n, m, R, seed = 4, 1, 3, SEEDS[0]
    assert RN.bits_formula(coin, n, m, R, fmask) == {0b0001: 39, 0b0010: 36}[fmask] - \
        (0 if coin == SM.RAND_LOCAL else 6)
    coins = RM.Coins(seed)
    loyal = [g for g in range(n) if not (fmask >> g) & 1]
    for t in range(16):
        ob = t & 1
        S = SM.stall_strategy(coin, n, m, R, fmask, ob, seed, t)
        assert 0 <= S < 1 << RN.bits_formula(coin, n, m, R, fmask)
        got = RN.history_message(coin, n, m, R, fmask, ob, RN.messages_of(coin, n, m, R, fmask, S))
        want = SM.history_message(n, m, R, coin, coins, t, fmask, ob)
        for p in range(R + 1):
            for g in loyal:
                assert [s[g] for s in got[p]] == [s[g] for s in want[p]], (t, p, g)
        assert RM.decided_of(n, fmask, ob, got) == RM.decided_of(n, fmask, ob, want)


@pytest.mark.parametrize("coin", COINS)
def test_reference_holds_every_decided_class(coin):
    """(10,3), f up to 10, R = 8: the reference of the GPU comparison holds trials decided
    in phase 1, decided later, unsafe and undecided, so that comparison cannot pass on
    one class."""
    dcd = SM.run(10, 3, 8, coin, seed=SEEDS[0], faulty_mode=O.FAULTY_RANDOM, f=10,
                 order_mode=O.ORDER_RANDOM, batch=B)[2]
    assert 1 in dcd and SM.UNSAFE in dcd and SM.UNDECIDED in dcd
    assert any(2 <= d <= 8 for d in dcd)


def test_in_bound_stall_and_beyond():
    """f = m: a local-coin trial with a faulty commander stays undecided until all loyal
    tosses fall alike, and is never unsafe.  f = m + 1: undecided for ever, with either
    coin, and still never unsafe."""
    n, m, R = 4, 1, 12
    kw = dict(seed=SEEDS[0], order_mode=O.ORDER_RANDOM, batch=128, form="plane")
    local = SM.run(n, m, R, SM.RAND_LOCAL, faulty_mode=O.FAULTY_EXACT, f=m, **kw)[2]
    assert SM.UNSAFE not in local and any(2 < d < SM.UNSAFE for d in local)
    for coin in COINS:
        ins = [(0b0011, t & 1) for t in range(64)]
        dcd = SM.run(n, m, R, coin, seed=SEEDS[0], batch=64, faulty=[i[0] for i in ins],
                     order=[i[1] for i in ins])[2]
        assert dcd == [SM.UNDECIDED] * 64


def test_k_rstall_kernels_do_not_spill():
    """The four k_rstall<GEN, COMMON> instantiations: no spilled vector register, no
    scratch memory; LDS only under the local coin, the four waves' 32 toss words."""
    import re
    import subprocess
    import tempfile

    import codeobj
    res = {k: v for k, v in codeobj.kernel_resources().items() if "k_rstall" in k}
    assert len(res) == 4, "k_rstall<GEN, COMMON> instantiations missing in libba_hip.so"
    for name, r in res.items():
        assert r["vgpr_spill"] == 0, (name, r)
    lds = []
    for co in codeobj.code_objects():
        with tempfile.NamedTemporaryFile(suffix=".co") as f:
            f.write(co)
            f.flush()
            notes = subprocess.run([f"{codeobj.LLVM}/llvm-readelf", "--notes", f.name], check=True,
                                   capture_output=True, text=True).stdout
        for blk in notes.split("- .agpr_count")[1:]:
            if "k_rstall" in re.search(r"\.name:\s+(\S+)", blk).group(1):
                assert int(re.search(r"\.private_segment_fixed_size:\s+(\d+)", blk).group(1)) == 0, blk
                lds.append(int(re.search(r"\.group_segment_fixed_size:\s+(\d+)", blk).group(1)))
    assert sorted(lds) == [0, 0, 4 * 8 * 32, 4 * 8 * 32]


def test_coin_calls():
    assert SM.coin_calls(10, 16, SM.RAND_LOCAL) == 160 and SM.coin_calls(10, 16, SM.RAND_COMMON) == 16
    assert SM.coin_calls(32, 250, SM.RAND_LOCAL) == 8000
    for bad in ((0, 1, 0), (33, 1, 0), (4, 0, 0), (4, 251, 0), (4, 1, 2)):
        assert SM.coin_calls(*bad) == 0
