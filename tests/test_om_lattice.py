"""The OM(m) lattice on the CPU: the anchor of tests/test_gpu_om_lattice.py.

The word-sliced port (oracle/ba_sliced.c), the GPU sweep's reference, equals the textbook
recursion (oracle/ba_oracle.c) on every lattice shape, depth 6 to 8 included; the given
inputs reach the root-tie path; the host ABI's geometry and engine choice equal the closed
forms and the restated dispatch rule; and the sweep lands on every kernel instantiation
the dispatch can reach.  No device needed."""
import numpy as np
import pytest

import om_lattice as OL
import oracle_c

# The recursion's cost grows with slots x trials.  Up to 2^16 slots a shape runs the full
# comparison of test_sliced_port_equals_recursion (batch 130, three mode triples); above,
# one ragged batch of 2^23 / slots trials, at least 3 and at most 67.
FULL_SLOTS = 1 << 16
BIG_WORK = 1 << 23


def big_batch(slots):
    return max(3, min(67, BIG_WORK // slots))


def _equal(n, m, B, **kw):
    d1, o1, c1 = oracle_c.run(n, m, B, **kw)
    d2, o2, c2 = oracle_c.sliced_run(n, m, B, **kw)
    assert len(c1) == 12
    assert np.array_equal(d1, d2) and np.array_equal(o1, o2) and c1 == c2, (n, m, B, c1, c2)


def test_lattice_shape():
    """One m per distinct effective depth, every (n, m_eff) within the slot cap, depths 6
    to 8 and every n present; the aliases have m > m_eff and a twin in the lattice."""
    assert len(set(OL.LATTICE)) == len(OL.LATTICE)
    assert {n for n, _ in OL.LATTICE} == set(range(1, 33))
    for n, me in OL.LATTICE:
        assert OL.m_eff(n, me) == me and OL.tree_slots(n, me) <= OL.SLOTS_SMALL
        assert OL.batches_of(n, me)[0] == OL.B_SMALL
    for n in range(1, 33):
        for me in range(0, OL.m_eff(n, 8) + 1):
            assert ((n, me) in OL.LATTICE) == (OL.tree_slots(n, me) <= OL.SLOTS_SMALL)
    assert {(8, 6), (9, 7), (10, 8), (11, 7), (12, 6), (16, 5), (32, 3)} <= set(OL.LATTICE)
    assert (11, 8) not in OL.LATTICE and (27, 4) not in OL.LATTICE
    for n, m in OL.ALIASES:
        assert m > OL.m_eff(n, m) and (n, OL.m_eff(n, m)) in OL.LATTICE
    assert OL.words_of(OL.B_SMALL) == 2 and OL.words_of(OL.B_WIDE) == 18
    assert OL.words_of(OL.B_LARGE) == 64 * 64 + 1


@pytest.mark.parametrize("n", range(1, 33))
def test_sliced_port_equals_recursion_on_lattice(n):
    """oracle_c.sliced_run == oracle_c.run in decisions, outcome bytes and the 12 counters
    on every lattice shape and alias of this n (n = 1: the port has no such tree and
    answers -4; the GPU sweep uses the recursion there)."""
    if n == 1:
        with pytest.raises(RuntimeError, match="rc=-4"):
            oracle_c.sliced_run(1, 0, 3, faulty=[0] * 3, order=[1] * 3)
        return
    for nn, m in OL.shapes_of(n) + OL.aliases_of(n):
        me = OL.m_eff(n, m)
        slots = OL.tree_slots(n, me)
        if slots <= FULL_SLOTS:
            for fmode, f, omode in [(1, (n - 1) // 3, 1), (2, min(n, m + 1), 2), (1, n, 1)]:
                _equal(n, m, 130, seed=12345 + n, faulty_mode=fmode, f=f, order_mode=omode,
                       order_value=2, first_trial=64 * 7)
            B = 130
        else:
            B = big_batch(slots)
            _equal(n, m, B, **OL.drawn_kw(n, me))
        _equal(n, m, B, **OL.given_kw(n, me, B))


@pytest.mark.parametrize("batch", OL.BATCHES + (OL.B_LARGE,))
def test_given_inputs_reach_root_ties(batch):
    """The given leg holds the all-faulty mask, OTHER orders, and -- for every odd n >= 3
    at depth >= 1 -- at least one undefined decision in the reference.  (OM(0) counts one
    vote per lieutenant: no tie exists at depth 0.)"""
    if batch == OL.B_LARGE:
        shapes = sorted(set(OL.LARGE_PER_TRIAL) | {s[:2] for s in OL.LARGE_EPI})
    else:
        shapes = [s for s in OL.LATTICE if batch in OL.batches_of(*s)]
    assert shapes
    for n, me in shapes:
        kw = OL.given_kw(n, me, batch)
        fm, oc = kw["faulty"], kw["order"]
        assert fm.dtype == np.uint32 and fm[1] == (1 << n) - 1 and (fm >> n == 0).all()
        assert (fm[0::4] == 1).all() and set(oc.tolist()) == {0, 1, 2}
        if n % 2 == 1 and n >= 3 and me >= 1:
            _, _, c = oracle_c.sliced_run(n, me, batch, **kw)
            assert c["undefined_decisions"] >= 1, (n, me, batch)


def test_drawn_inputs():
    for n, me in OL.LATTICE:
        kw = OL.drawn_kw(n, me)
        assert kw["faulty_mode"] == 1 and kw["order_mode"] == 1 and kw["f"] == (n - 1) // 3 + 1
        assert kw["first_trial"] > 0 and kw["first_trial"] % 64 == 0


def test_host_geometry_equals_closed_forms():
    """ba_tree_slots / ba_level_slots for all 288 (n, m), and 0 outside the domain."""
    from ba_amd import lib as L
    lib = L.load()
    for n in range(1, 33):
        for m in range(0, 9):
            me = OL.m_eff(n, m)
            assert lib.ba_tree_slots(n, m) == OL.tree_slots(n, me), (n, m)
            for k in range(0, 10):
                want = OL.level_slots(n, me, k) if k <= me else 0
                assert lib.ba_level_slots(n, m, k) == want, (n, m, k)
    for n, m in [(0, 0), (0, 3), (33, 0), (33, 8), (10, 9), (32, 9), (1, 9), (2 ** 32 - 1, 1)]:
        assert lib.ba_tree_slots(n, m) == 0, (n, m)
        assert lib.ba_level_slots(n, m, 0) == 0, (n, m)
    # closed forms against figures worked by hand
    assert OL.tree_slots(10, 3) == 9 + 72 + 504 + 3024 and OL.tree_slots(1, 0) == 0
    assert OL.tree_slots(32, 8) == sum(OL.perm(31, k) for k in range(1, 10))
    assert OL.perm(31, 9) == 31 * 30 * 29 * 28 * 27 * 26 * 25 * 24 * 23 > 1 << 40


def test_engine_for_equals_restated_rule():
    from ba_amd import lib as L
    lib = L.load()
    code = {"FUSED": L.ENGINE_FUSED, "LEVELS": L.ENGINE_LEVELS}
    for n, m in OL.LATTICE + OL.ALIASES:
        assert lib.ba_engine_for(n, m) == code[OL.engine_for(n, OL.m_eff(n, m))], (n, m)
    # the trees that plan at depth 5, and none at depth 6
    assert [s for s in OL.LATTICE if s[1] == 5 and OL.plan_fused(*s)] == [(7, 5), (8, 5)]
    assert not any(OL.plan_fused(n, 6) for n in range(8, 33))


def test_reach_is_complete():
    """The sweep lands on every instantiation the dispatch can reach at all."""
    reach = OL.reach()
    want = set()
    want |= {("k_om3w", n) for n in range(5, 15)} | {("k_om3wt", 10)}
    want |= {("k_om4w", n) for n in range(6, 15)}
    want |= {("k_leaf", s) for s in range(2, 13)} | {("k_leaf_up", s) for s in range(2, 13)}
    want |= {("k_relay_top", k) for k in range(0, 7)} | {("k_relay_fallback",)}
    want |= {("k_tail", n) for n in range(4, 17)}
    want |= {("k_epilogue_w", n) for n in range(4, 17)} | {("k_epilogue_bs", 4), ("k_epilogue_bs", 5)}
    want |= {("k_majority", p) for p in range(2, 6)} | {("k_epilogue", p) for p in range(1, 6)}
    want |= {("k_cascade", 16, 5), ("k_cascade", 16, 4)}
    # k_fused<S> at every depth it plans for
    fused = {(n - me, me) for n in range(1, 33) for me in range(0, OL.m_eff(n, 8) + 1)
             if OL.plan_fused(n, me)}
    assert {s for s, _ in fused} == set(range(2, 13))
    assert {me for _, me in fused} == {2, 3, 4, 5}
    assert {(12, 2), (12, 3), (2, 5), (3, 5)} <= fused
    want |= {("k_fused", s, me) for s, me in fused}
    assert want <= reach, sorted(want - reach)
    # and nothing any call reaches is left out, but the cascade shapes that only
    # ENGINE_LEVELS in its default environment runs (tests/test_gpu_cascade.py)
    other = OL.reachable() - reach
    assert other == set(), sorted(other)
    levels_only = {("k_cascade", n, me) for n, me in OL.CASCADE_SHAPES if OL.use_cascade(n, me)}
    assert levels_only == {("k_cascade", 16, 5), ("k_cascade", 16, 4), ("k_cascade", 10, 3),
                           ("k_cascade", 9, 4), ("k_cascade", 8, 5)}
    # compiled, never dispatched
    assert ("k_majority", 1) not in OL.reachable()
    assert not OL.use_cascade(16, 3)  # S = 13 > 12: k_cascade<16, 3> cannot run
    assert not any(OL.plan_fused(n, me) for n in range(17, 33) for me in range(0, 9))  # k_fused's L >= 16 root branch
