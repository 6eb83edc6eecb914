"""CPU tests of SM(m), signed messages (docs/SEMANTICS.md §6): the reference model
(tests/sm_model.py) against the figures the contract was checked with and against
Lamport's theorem, its two forms against each other, the host-only coin-call
count, and the built kernels' register spills."""
import pytest

import ba_oracle as O
import sm_model as S

# (n, m, f, trials, violations, trials with some |V| = 2): seed 7, FAULTY_EXACT,
# ORDER_RANDOM, trials 0..T-1; a violation is IC1 or IC2 failing
TABLE = [(4, 1, 1, 300, 0, 54), (4, 1, 2, 300, 12, 108), (5, 2, 2, 300, 0, 105),
         (5, 2, 3, 300, 0, 158), (7, 3, 3, 200, 0, 89), (6, 0, 1, 100, 9, 9),
         (4, 5, 3, 200, 0, 104)]
THEOREM = [(3, 1), (4, 1), (4, 2), (5, 2), (7, 3)]


def _table_run(n, m, f, T, form="chain"):
    return S.run(n, m, seed=7, faulty_mode=O.FAULTY_EXACT, f=f, order_mode=O.ORDER_RANDOM, batch=T,
                 form=form)


def _theorem_run(n, m, form="chain"):
    return S.run(n, m, seed=11, faulty_mode=O.FAULTY_RANDOM, f=m, order_mode=O.ORDER_RANDOM,
                 batch=256, form=form)


def test_coins_are_the_oracle_lie_stream():
    c = S.Coins(0xBA5EED)
    for t in (0, 5, 64, 777, (1 << 38) + 3):
        for k in range(4):
            for x in range(9):
                assert c(t, k, x) == O.lie(0xBA5EED, t, 64 + k, x)


@pytest.mark.parametrize("n,m,f,T,viol,two", TABLE)
def test_model_reproduces_contract_table(n, m, f, T, viol, two):
    dec, out, vs, cnt = _table_run(n, m, f, T)
    assert S.violations(out) == viol
    assert S.two_valued(vs) == two
    assert cnt["trials"] == T and cnt["undefined_decisions"] == 0
    assert cnt["faulty_total"] == f * T
    assert cnt["in_bound"] == (T if f <= m else 0)
    assert cnt["bound_violations"] == (viol if f <= m else 0)


@pytest.mark.parametrize("n,m", THEOREM)
def test_no_violation_within_the_bound(n, m):
    dec, out, vs, cnt = _theorem_run(n, m)
    assert S.violations(out) == 0
    assert cnt["in_bound"] == 256 and cnt["bound_violations"] == 0
    assert cnt["agreement"] == 256 and cnt["validity"] == cnt["validity_applicable"]


@pytest.mark.parametrize("n,m,f,T,viol,two", TABLE)
def test_plane_form_equals_chain_form_on_table(n, m, f, T, viol, two):
    assert _table_run(n, m, f, T, "plane") == _table_run(n, m, f, T)


@pytest.mark.parametrize("n,m", THEOREM)
def test_plane_form_equals_chain_form_on_theorem_inputs(n, m):
    assert _theorem_run(n, m, "plane") == _theorem_run(n, m)


@pytest.mark.parametrize("n,m", [(4, 1), (5, 2), (7, 3)])
def test_plane_form_equals_chain_form_across_2_38(n, m):
    """192 trials from first_trial = 2^38 - 64: the plane form keys its coin words
    by the trial word (2^32 - 1, then 2^32 and 2^32 + 1 with the upper counter
    word set), the chain form by the trial; every general may be faulty."""
    kw = dict(seed=0x5157ED0123456789, faulty_mode=O.FAULTY_RANDOM, f=n, order_mode=O.ORDER_RANDOM,
              first_trial=2**38 - 64, batch=192)
    chain = S.run(n, m, form="chain", **kw)
    assert S.run(n, m, form="plane", **kw) == chain
    assert chain[3]["trials"] == 192 and chain[0][:64] != chain[0][64:128] != chain[0][128:]


def test_decision_rule_and_vset_packing():
    # a loyal commander and no traitor: V = {order} everywhere, in both packings
    dec, out, vs, cnt = S.run(5, 2, seed=3, faulty=[0, 0, 0], order=[1, 0, 2], batch=3)
    assert dec == [0b01010101, 0, 0]
    assert vs == [0b01010101, 0b10101010, 0b10101010]
    assert [o & 3 for o in out] == [O.Q_ATTACK, O.Q_RETREAT, O.Q_RETREAT]
    assert S.choice(set()) == S.choice({0}) == S.choice({0, 1}) == O.RETREAT
    assert S.choice({1}) == O.ATTACK


def test_coin_calls_formula():
    from ba_amd import lib as L
    for n in range(1, 33):
        for m in range(0, 9):
            Lt, me = n - 1, O.effective_depth(n, m)
            want = Lt + me * Lt * (Lt - 1)
            assert L.sm_coin_calls(n, m) == want == S.coin_calls(n, m), (n, m)
    assert L.sm_coin_calls(10, 3) == 225


def test_k_sm_kernels_do_not_spill():
    import codeobj
    res = {k: v for k, v in codeobj.kernel_resources().items() if "k_sm" in k}
    assert len(res) >= 1, "no k_sm kernel in libba_hip.so"
    for name, r in res.items():
        assert r["vgpr_spill"] == 0, (name, r)
