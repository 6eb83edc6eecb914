"""GPU census of the enumeration kernels (tests/enum_census.py, tests/golden/enum_census.json):
every reachable instantiation of k_kenum<PROTO, N>, k_renum<COMMON, N> and k_enum<ME>
against its model at strategies where the free bits are live, so that a plane read at a
wrong index changes what is compared.  Every comparison is exact: decisions, outcome
bytes, `decided` bytes, all 12 counters, the witness and, for RAND, the stats.  The
fixture is read, never searched; tests/test_enum_census.py holds it to the models."""
import numpy as np
import pytest

import ba_oracle as O
import enum_census as C
import enum_model as EM
import kenum_model as KM
import renum_model as RM

pytestmark = pytest.mark.gpu

A, R, OTHER = O.ATTACK, O.RETREAT, O.OTHER
DOC = C.load()
INSTS = list(dict.fromkeys((r["family"], r["sel"]) for r in DOC["cases"]))


def gpu(engine, case, first, count):
    """[first, first + count) of the case with every per-strategy output."""
    f, n, m, R_, F, o = case
    kw = dict(first=first, count=count, want_decisions=True, want_outcome=True)
    if f in C.PROTO:
        return engine.run_kenum(C.PROTO[f], n, m, F, o, **kw)
    if f in C.COIN:
        return engine.run_renum(C.COIN[f], n, m, R_, F, o, want_decided=True, **kw)
    return engine.run_enum(n, m, F, o, **kw)


def model(case, first, count):
    """(decisions, outcome, decided or None, counters, witness or None, stats or None) of
    the range, one strategy at a time (kenum, renum) or on the level arrays (OM(m))."""
    f, n, m, R_, F, o = case
    dcd = st = None
    if f in C.PROTO:
        dec, out, cnt, wit = KM.run_message(C.PROTO[f], n, m, F, o, first, count)
    elif f in C.COIN:
        dec, out, dcd, cnt, wit, st = RM.run_message(C.COIN[f], n, m, R_, F, o, first, count)
        dcd = np.array(dcd, np.uint8)
    else:
        dec, out, cnt, wit = EM.run(n, m, F, o, first, count)
        wit = None if wit == EM.NO_WITNESS else wit
    return np.array(dec, np.uint64), np.array(out, np.uint8), dcd, cnt, wit, st


def same(a, b, what):
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape, f"{what}: shape {a.shape} != {b.shape}"
    if not np.array_equal(a, b):
        idx = np.nonzero(a != b)[0]
        raise AssertionError(f"{what}: {len(idx)} mismatches, first at {idx[:5].tolist()}: "
                             f"got {a[idx[:5]].tolist()} want {b[idx[:5]].tolist()}")


def check_range(engine, case, first, count, what):
    what = f"{what} {tuple(case)} [{first}, +{count})"
    res = gpu(engine, case, first, count)
    dec, out, dcd, cnt, wit, st = model(case, first, count)
    same(res.decisions, dec, f"{what} decisions")
    same(res.outcome, out, f"{what} outcome")
    assert len(cnt) == 12 and cnt["trials"] == count
    assert {k: res.counters[k] for k in cnt} == cnt, what
    assert res.witness == wit, what
    if case.family in C.COIN:
        same(res.decided, dcd, f"{what} decided")
        assert res.stats == st, (what, res.stats, st)
        assert st["unsafe"] + st["undecided"] + sum(st["decided_in"]) == cnt["trials"], what
    return res


class Windows:
    """The 64-strategy windows of one case on the GPU, each launched once."""

    def __init__(self, engine, case):
        self.engine, self.case, self.size = engine, case, 1 << C.bits(case)
        self.res = {}

    def at(self, S):
        first = S & ~63
        if first not in self.res:
            self.res[first] = gpu(self.engine, self.case, first, min(64, self.size - first))
        r, i = self.res[first], S - first
        got = (int(r.decisions[i]), int(r.outcome[i]))
        return got + (int(r.decided[i]),) if self.case.family in C.COIN else got


@pytest.mark.parametrize("inst", INSTS, ids=lambda i: C.kernel_name(*i))
def test_instantiation_equals_its_model_where_the_free_bits_are_live(engine, inst):
    recs = [r for r in DOC["cases"] if (r["family"], r["sel"]) == inst]
    assert recs
    for rec in recs:
        case, B = C.case_of(rec), rec["B"]
        size = 1 << B
        # 1. every recorded strategy and its partner across every recorded live bit
        win = Windows(engine, case)
        for S, bs in rec["live"]:
            base = C.evaluate(case, S)
            assert win.at(S) == base, (rec["kernel"], tuple(case), S)
            for b in bs:
                want = C.evaluate(case, S ^ (1 << b))
                assert want != base  # the bit is live: the partner is another output
                assert win.at(S ^ (1 << b)) == want, (rec["kernel"], tuple(case), S, b)
        # 2. whole windows: the bottom and the top of the space and a live window, or the
        # whole space up to 2^12; arrays, counters, witness, stats
        if B <= 12:
            check_range(engine, case, 0, size, rec["kernel"])
            continue
        firsts = [0, size - 64] + [S & ~63 for S, _ in rec["live"][:1]]
        for first in dict.fromkeys(firsts):
            check_range(engine, case, first, 64, rec["kernel"])


# N = 1 has no lieutenant (no plane in LDS although the outputs are on, needed = 1), N = 2
# one (needed = n - 1): every F, every order code, whole spaces.
SMALL = [(f, N) for f in (C.KING, C.KING3, C.LOCAL, C.COMMON, C.OM) for N in (1, 2)]


@pytest.mark.parametrize("family,N", SMALL, ids=lambda v: str(v))
def test_one_and_two_generals_whole_spaces(engine, family, N):
    ran = 0
    for m in (0, 1, 2):
        for R_ in ((1, 2) if family in C.COIN else (0,)):
            for F in range(1 << N):
                for o in (A, R, OTHER):
                    case = C.Case(family, N, m, R_, F, o)
                    B = C.bits(case)
                    assert B <= 9
                    res = check_range(engine, case, 0, 1 << B, f"{family} N={N}")
                    assert res.counters["trials"] == 1 << B
                    ran += 1
    assert ran == 3 * (2 if family in C.COIN else 1) * (1 << N) * 3


def test_unreachable_k_enum_depths_are_refused(engine):
    """k_enum<6>, <7> and <8> need n >= 8, 9 and 10, whose slot maps (13,699 slots and
    more) do not fit the 4,096 bytes of LDS the kernel gives them: the API says so, for
    the smallest space (F = {0}: n - 1 bits) as for any other."""
    from ba_amd import lib as L
    for me in (6, 7, 8):
        for n in (me + 2, me + 3):
            assert O.effective_depth(n, me) == me and C.tree_slots(n, me) > C.MAX_SLOTS
            with pytest.raises(L.BAError) as e:
                engine.run_enum(n, me, 0b1, A, first=0, count=64)
            assert e.value.code == L.ETOOBIG
    # the deepest reachable one runs
    res = engine.run_enum(7, 5, 0b1, A)
    assert res.counters["trials"] == 64
