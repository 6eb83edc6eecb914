"""CPU tests of OM(m) under scripted traitor policies (docs/SEMANTICS.md §7): the
reference model (tests/adv_model.py), its two forms against each other, Lamport's
theorem and its converse on exhaustive faulty sets, the pinned violation counts,
the host-only path count and the built kernels' resources."""
import re
import subprocess
import tempfile

import pytest

import adv_model as A
import ba_oracle as O

# (n, m, f): (cases, violations SPLIT, FLIP, ANTI) over every f-subset x {retreat, attack}
PINNED = {(3, 1, 1): (6, 2, 4, 4), (4, 1, 2): (12, 7, 6, 10), (5, 1, 2): (20, 18, 12, 20),
          (6, 1, 3): (40, 34, 20, 38), (7, 2, 3): (70, 56, 40, 58), (7, 2, 4): (70, 60, 0, 66),
          (4, 2, 1): (8, 3, 3, 3), (6, 2, 2): (30, 10, 10, 10)}


def _all_rows(n):
    return [(fm, oc) for fm in range(1 << n) for oc in (0, 1, 2)]


@pytest.mark.parametrize("policy", A.POLICIES)
@pytest.mark.parametrize("n,m", [(3, 1), (4, 1), (4, 2), (5, 2), (6, 2)])
def test_both_forms_agree_on_every_mask_and_order(n, m, policy):
    rows = _all_rows(n)
    kw = dict(batch=len(rows), faulty=[r[0] for r in rows], order=[r[1] for r in rows])
    lev = A.run(n, m, policy, form="levels", **kw)
    assert lev == A.run(n, m, policy, form="rec", **kw)
    assert lev[2]["trials"] == 3 << n


@pytest.mark.parametrize("n,m,cases", [(4, 1, 10), (5, 1, 12), (7, 2, 58), (10, 3, 352)])
def test_theorem_no_policy_breaks_om_within_the_bound(n, m, cases):
    """n > 3m, every faulty set with |F| <= me, both orders: IC1 and IC2 hold."""
    me = O.effective_depth(n, m)
    assert n > 3 * me
    for policy in A.POLICIES:
        total = 0
        for f in range(me + 1):
            c, viol, bad = A.census(n, m, policy, f)
            assert viol == 0, (policy, f, bad[:3])
            total += c
        assert total == cases


@pytest.mark.parametrize("shape", sorted(PINNED))
def test_pinned_violation_counts(shape):
    n, m, f = shape
    cases, *want = PINNED[shape]
    for policy, w in zip(A.POLICIES, want):
        c, viol, _ = A.census(n, m, policy, f)
        assert (c, viol) == (cases, w), (shape, A.POLICY_NAMES[policy])


def test_rec_form_reproduces_a_pinned_row():
    assert A.census(5, 1, A.ANTI, 2, form="rec")[:2] == (20, 20)
    assert A.census(7, 2, A.FLIP, 4, form="rec")[:2] == (70, 0)


def test_flip_at_n3_breaks_exactly_when_the_traitor_is_a_lieutenant():
    c, viol, bad = A.census(3, 1, A.FLIP, 1)
    assert (c, viol) == (6, 4)
    assert sorted(bad) == [(fm, oc) for fm in (0b010, 0b100) for oc in (0, 1)]


@pytest.mark.parametrize("policy", A.POLICIES)
def test_no_traitor_equals_the_oracle(policy):
    for n, m in [(1, 0), (2, 1), (3, 1), (4, 0), (4, 1), (5, 2), (7, 3), (7, 8)]:
        order = [0, 1, 2, 1]
        kw = dict(batch=4, faulty=[0] * 4, order=order, first_trial=64)
        for form in ("levels", "rec"):
            assert A.run(n, m, policy, form=form, **kw) == O.run(n, m, seed=5, **kw), (n, m, form)


def test_drawn_inputs_are_the_oracles():
    """Same seed, same synthetic faulty sets and orders as an OM run (§4)."""
    kw = dict(seed=0xBA5EED, faulty_mode=O.FAULTY_RANDOM, f=5, order_mode=O.ORDER_RANDOM, batch=40)
    _, _, cnt = A.run(5, 2, A.SPLIT, **kw)
    _, _, ref = O.run(5, 2, **kw)
    for k in ("trials", "faulty_total", "validity_applicable", "in_bound"):
        assert cnt[k] == ref[k]


def test_paths_formula_and_cap():
    from ba_amd import lib as L
    for n in range(0, 35):
        for m in range(0, 10):
            want = 0
            if 1 <= n <= 32 and m <= 8:
                want = 1
                for i in range(O.effective_depth(n, m)):
                    want *= n - 2 - i
            assert L.adv_paths(n, m) == want == A.paths(n, m), (n, m)
    assert L.adv_paths(10, 3) == 336 and L.adv_paths(2, 5) == 1 and L.adv_paths(1, 0) == 1
    for n, m in [(16, 6), (32, 4), (12, 8)]:
        assert L.adv_paths(n, m) <= A.PATH_CAP, (n, m)
    for n, m in [(32, 5), (16, 7), (16, 8)]:
        assert L.adv_paths(n, m) > A.PATH_CAP, (n, m)


def test_k_adv_kernels_use_no_spill_and_no_scratch():
    import codeobj
    res = {k: v for k, v in codeobj.kernel_resources().items() if "k_adv" in k}
    assert len(res) == 18, sorted(res)  # me = 0..8 x {table policies, FLIP}
    for name, r in res.items():
        assert r["vgpr_spill"] == 0, (name, r)
    # the private segment (scratch) of every k_adv, from the same metadata notes
    seen = 0
    for co in codeobj.code_objects():
        with tempfile.NamedTemporaryFile(suffix=".co") as f:
            f.write(co)
            f.flush()
            notes = subprocess.run([f"{codeobj.LLVM}/llvm-readelf", "--notes", f.name], check=True,
                                   capture_output=True, text=True).stdout
        for blk in notes.split("- .agpr_count")[1:]:
            name = re.search(r"\.name:\s+(\S+)", blk).group(1)
            if "k_adv" in name:
                seen += 1
                assert int(re.search(r"\.private_segment_fixed_size:\s+(\d+)", blk).group(1)) == 0, name
    assert seen == 18

