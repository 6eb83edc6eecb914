"""OM(m) across every shape the engines dispatch on, depth 6 to 8 included.

Every shape of tests/om_lattice.py runs on every engine variant that applies to it, at a
two-word and an eighteen-word batch, with drawn and with given inputs.  Each run is
checked three ways: decisions, outcome bytes and the 12 counters equal the word-sliced
CPU port bit for bit (oracle_c.sliced_run, which tests/test_om_lattice.py holds to the
recursion on the same shapes); the profiled kernel names are exactly those the restated
dispatch rule names, so a shape cannot slide to another kernel unnoticed; and an
m > m_eff alias equals its twin.  Beside the lattice: the big-batch epilogues at every n
they are compiled for, and the tree that is too big for any engine."""
import numpy as np
import pytest

import om_lattice as OL
import oracle_c
from test_gpu import same

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def engine_noleaf():
    """LEVELS with materialised leaves: BA_NO_LEAF_FUSION is read at ba_ctx_create."""
    from ba_amd.lib import Engine
    with pytest.MonkeyPatch.context() as mp:
        mp.setenv("BA_NO_LEAF_FUSION", "1")
        eng = Engine(0)
    yield eng
    eng.close()


def reference(n, m, batch, kw):
    run = oracle_c.sliced_run if n >= 2 else oracle_c.run  # the port has no n = 1 tree
    return run(n, m, batch, **kw)


def run_profiled(eng, n, m, batch, engine, kw):
    eng.profile(True)
    try:
        res = eng.run(n, m, batch, engine=engine, **kw)
        names = set(eng.profile_read())
    finally:
        eng.profile(False)
    return res, names


def check(res, ref, names, want, tag):
    od, oo, oc = ref
    same(res.decisions, od, "decisions " + tag)
    same(res.outcome, oo, "outcome " + tag)
    assert {k: res.counters[k] for k in oc} == oc, tag
    got = OL.normalise(names)
    assert got == want.names, f"{tag}: launched {sorted(got)}, the rule says {sorted(want.names)}"
    assert got <= OL.NAMES


ENV = {"V1": {}, "V2": {"BA_NO_CASCADE": "1"}, "V3": {}, "V4": {"BA_FUSED_KIND": "2"},
       "V5": {"BA_OM3W_TABLE": "0"}}
SWITCHES = ["BA_NO_CASCADE", "BA_FUSED_KIND", "BA_OM3W_TABLE", "BA_NO_INPUT_FUSION", "BA_NO_LEAF_UP",
            "BA_NO_TAIL", "BA_NO_TOP_RELAY", "BA_NO_EPILOGUE_W", "BA_CASC_TWO", "BA_CASC_CO",
            "BA_CASC_WTOP", "BA_CASC_MTOP", "BA_CASC_CHECK", "BA_WAVE_MAX_BLOCKS"]


@pytest.mark.parametrize("n", range(1, 33))
def test_lattice_vs_sliced_port(engine, engine_noleaf, monkeypatch, n):
    from ba_amd import lib as L
    eng_code = {"V1": L.ENGINE_AUTO, "V2": L.ENGINE_LEVELS, "V3": L.ENGINE_LEVELS,
                "V4": L.ENGINE_FUSED, "V5": L.ENGINE_AUTO}
    runs = 0
    for nn, m in OL.shapes_of(n) + OL.aliases_of(n):
        me = OL.m_eff(n, m)
        for batch in OL.batches_of(n, me):
            legs = {"drawn": OL.drawn_kw(n, me), "given": OL.given_kw(n, me, batch)}
            refs = {leg: reference(n, m, batch, kw) for leg, kw in legs.items()}
            if m != me:  # an alias: the twin's reference too
                for leg, kw in legs.items():
                    twin = reference(n, me, batch, kw)
                    same(refs[leg][0], twin[0], f"alias reference n={n} m={m}")
                    assert refs[leg][2] == twin[2]
            for v in OL.VARIANTS:
                if not OL.applies(v, n, me):
                    continue
                for s in SWITCHES:
                    monkeypatch.delenv(s, raising=False)
                for k, val in ENV[v].items():
                    monkeypatch.setenv(k, val)
                want = OL.expect(n, me, v, OL.words_of(batch))
                eng = engine_noleaf if v == "V3" else engine
                for leg, kw in legs.items():
                    tag = f"n={n} m={m} {v} batch={batch} {leg}"
                    res, names = run_profiled(eng, n, m, batch, eng_code[v], kw)
                    check(res, refs[leg], names, want, tag)
                    runs += 1
    assert runs >= 4  # V1 and V2, two legs, at the very least


LARGE = ([(n, m, epi_w) for n, m, epi_w in OL.LARGE_EPI] + [(n, m, True) for n, m in OL.LARGE_PER_TRIAL])


@pytest.mark.parametrize("n,m,epi_w", LARGE)
def test_large_batch_epilogues(engine, monkeypatch, n, m, epi_w):
    """4097 words, ENGINE_LEVELS, given inputs with OTHER orders, dense sets and
    commander-only sets: k_epilogue_w and (BA_NO_EPILOGUE_W=1) k_epilogue_bs at every n
    they are compiled for, and the per-trial k_epilogue<P> at scale where neither applies
    -- (17, 2) with 16 lieutenants: root ties, five count planes, many groups."""
    from ba_amd import lib as L
    for s in SWITCHES:
        monkeypatch.delenv(s, raising=False)
    monkeypatch.setenv("BA_NO_EPILOGUE_W", "0" if epi_w else "1")
    me = OL.m_eff(n, m)
    kw = OL.given_kw(n, me, OL.B_LARGE)
    want = OL.expect(n, me, "LEVELS", OL.words_of(OL.B_LARGE), epi_w=epi_w)
    kind = {k for k, *_ in want.inst if k.startswith("k_epilogue")}
    assert kind == ({"k_epilogue_w" if epi_w else "k_epilogue_bs"} if 4 <= n <= 16 else {"k_epilogue"})
    ref = reference(n, m, OL.B_LARGE, kw)
    if n % 2 == 1:
        assert ref[2]["undefined_decisions"] >= 1
    res, names = run_profiled(engine, n, m, OL.B_LARGE, L.ENGINE_LEVELS, kw)
    check(res, ref, names, want, f"n={n} m={m} epi_w={epi_w}")


def test_too_big_is_refused_on_the_host(engine):
    """(32, 8) has levels above 2^31 slots: BA_ETOOBIG before anything is launched, and the
    ctx works on."""
    from ba_amd import lib as L
    engine.profile(True)
    try:
        with pytest.raises(L.BAError) as ei:
            engine.run(32, 8, 1, faulty=[0], order=[1])
        assert ei.value.code == L.ETOOBIG
        assert engine.profile_read() == {}
    finally:
        engine.profile(False)
    kw = OL.given_kw(7, 2, OL.B_SMALL)
    res, names = run_profiled(engine, 7, 2, OL.B_SMALL, L.ENGINE_AUTO, kw)
    check(res, reference(7, 2, OL.B_SMALL, kw), names, OL.expect(7, 2, "V1", 2), "after ETOOBIG")
