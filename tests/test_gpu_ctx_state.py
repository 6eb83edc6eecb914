"""The state a ba_ctx carries from one launch to the next (include/ba.h, "Conventions"):
the counter sink's replicas ("zero between launches"), the WAVE engines' task counter
behind them, the scratch, the ordering event and the profile -- under graph capture
and replay, and under calls of one ctx from two streams.

Every comparison is exact: decision words, outcome bytes, settled / vsets bytes and
the 12 counters, against the CPU references the per-entry files use (the oracle for
OM(m) and the table mode, the models for SM, ADV, KING, KING3 and ENUM).

Graphs are single-stream and linear, captured with torch.cuda.graph on a side stream
after the identical eager call (ba.h: capture only after an eager call of the same
size), each from an Engine of its own, and replayed one at a time per ctx."""
import functools

import numpy as np
import pytest

import adv_model as A
import ba_oracle as O
import enum_model as E
import king3_model as K3
import king_model as K
import oracle_c
import sm_model as S
from test_gpu import same
from test_gpu_adv import adv_units
from wave_shape import OM3W_BPC, cu_count, om4w_words, wave_shape

pytestmark = pytest.mark.gpu

SEED = 0xC7C57A7E
FIRST = 64 * 21
B69 = 64 * 68 + 37      # 69 words: 72 reporting waves of k_sm / k_king / k_king3 (four-wave blocks)
B_OM3 = 64 * 8 * 70 + 37  # 71 tasks of k_om3wt: 18 blocks, one reporting unit each
B_OM3_REP = 64 * 8 * 4 * 65 + 37  # 261 tasks: 66 blocks, more than the sink's 64 replicas
B_LEV = 64 * 70 + 9
B_OM4 = 64 * 10 * 11 + 37  # (9, 4): 12 tasks of 10 words


def wave_units(B):
    return 4 * (((B + 63) // 64 + 3) // 4)


# --- references (computed once, shared) ------------------------------------------------
def om_kw(n, first=FIRST):
    return dict(seed=SEED + n, faulty_mode=O.FAULTY_RANDOM, f=(n - 1) // 3 + 1, order_mode=O.ORDER_RANDOM,
                first_trial=first)


def model_kw(n, first=FIRST):
    return dict(seed=SEED + n, faulty_mode=O.FAULTY_RANDOM, f=n, order_mode=O.ORDER_RANDOM, first_trial=first)


@functools.lru_cache(maxsize=None)
def ref_om(n, m, B, first=FIRST):
    od, oo, cnt = oracle_c.run(n, m, B, **om_kw(n, first))
    return {"decisions": od, "outcome": oo}, cnt


@functools.lru_cache(maxsize=None)
def ref_om_inputs(n, B, first=FIRST):
    kw = om_kw(n, first)
    return oracle_c.sliced_gen(n, B, seed=kw["seed"], faulty_mode=kw["faulty_mode"], f=kw["f"],
                               order_mode=kw["order_mode"], first_trial=first)


@functools.lru_cache(maxsize=None)
def ref_sm(n, m, B, first=FIRST):
    dec, out, vs, cnt = S.run(n, m, batch=B, **model_kw(n, first))
    return {"decisions": np.array(dec, np.uint64), "outcome": np.array(out, np.uint8),
            "vsets": np.array(vs, np.uint64)}, cnt


@functools.lru_cache(maxsize=None)
def ref_adv(n, m, policy, B, first=FIRST):
    dec, out, cnt = A.run(n, m, policy, batch=B, **model_kw(n, first))
    return {"decisions": np.array(dec, np.uint64), "outcome": np.array(out, np.uint8)}, cnt


@functools.lru_cache(maxsize=None)
def ref_king(kind, n, m, policy, B, first=FIRST):
    dec, out, stl, cnt = (K if kind == "king" else K3).run(n, m, policy, batch=B, **model_kw(n, first))
    return {"decisions": np.array(dec, np.uint64), "outcome": np.array(out, np.uint8),
            "settled": np.array(stl, np.uint8)}, cnt


@functools.lru_cache(maxsize=None)
def ref_enum(n, m, F, o, first, count):
    dec, out, cnt, wit = E.run(n, m, F, o, first, count)
    return {"decisions": np.array(dec, np.uint64), "outcome": np.array(out, np.uint8)}, cnt, wit


@functools.lru_cache(maxsize=None)
def ref_table(n, B):
    from ba_amd import lib as L
    rng = np.random.default_rng(n * 1000 + B)
    seeds = rng.integers(0, 1 << 63, B, dtype=np.uint64)
    faulty = (rng.integers(0, 1 << n, B, dtype=np.int64) & rng.integers(0, 1 << n, B, dtype=np.int64)
              ).astype(np.uint32)
    order = rng.choice([0, 1, 2], B).astype(np.uint8)
    tab, _ = L.mt_table(n, 1, seeds, faulty)
    od, oo, cnt = oracle_c.run(n, 1, B, lie_mode=1, faulty=faulty, order=order, table=tab)
    return seeds, faulty, order, {"table": tab, "decisions": od, "outcome": oo}, cnt


# --- one library call (or a pair on one stream) with its buffers and reference ----------
class Call:
    """issue(engine, stream handle) enqueues the call; outs: name -> device tensor it
    writes; want: name -> the reference array; ref_cnt: the 12 reference counters."""

    def __init__(self, name, B, outs, want=None, cnt_dict=None):
        import torch
        from ba_amd import lib as L
        self.name, self.B, self.outs, self.want = name, B, outs, want
        self.ref_cnt = None if cnt_dict is None else [cnt_dict[k] for k in L.COUNTER_NAMES]
        self.cnt = torch.zeros(16, dtype=torch.int64, device="cuda")
        self.issue = None

    def poison(self):
        """decisions -1, bytes 254 (on the current stream)."""
        import torch
        for t in self.outs.values():
            t.fill_(254 if t.dtype == torch.uint8 else -1)

    def read(self):
        return ({k: t.cpu().numpy().view(np.uint8 if t.element_size() == 1 else
                                         (np.uint32 if t.element_size() == 4 else np.uint64))
                 for k, t in self.outs.items()}, self.cnt.cpu().tolist())

    def verify(self, times, what):
        """Every output equals the reference; the counters equal times x the reference."""
        got, cnt = self.read()
        for k, want in self.want.items():
            same(got[k].reshape(-1), np.asarray(want).reshape(-1), f"{self.name}, {what}: {k}")
        assert cnt[:12] == [times * v for v in self.ref_cnt], f"{self.name}, {what}: counters x{times}"
        assert cnt[12:] == [0, 0, 0, 0], f"{self.name}, {what}"

    def adopt(self):
        """The reference of a call too large for its model: what the call gave alone."""
        got, cnt = self.read()
        self.want, self.ref_cnt = {k: v.copy() for k, v in got.items()}, cnt[:12]
        assert cnt[12:] == [0, 0, 0, 0], self.name


def _bufs(B, **extra):
    import torch
    outs = {"decisions": torch.empty(B, dtype=torch.int64, device="cuda"),
            "outcome": torch.empty(B, dtype=torch.uint8, device="cuda")}
    for k, dt in extra.items():
        outs[k] = torch.empty(B, dtype=dt, device="cuda")
    return outs


def om_call(n, m, B, engine_sel=0, staged=False, first=FIRST, ref=True):
    """ba_run_trials_device drawing its inputs, or (staged) ba_gen_inputs_device + the
    GIVEN run on one stream: bench.py's pattern."""
    import torch
    from ba_amd import lib as L
    kw = om_kw(n, first)
    outs = _bufs(B, **({"faulty": torch.int32, "order": torch.uint8} if staged else {}))
    want, cnt = ref_om(n, m, B, first) if ref else (None, None)
    if staged and ref:
        fm, oc = ref_om_inputs(n, B, first)
        want = dict(want, faulty=fm, order=oc)
    c = Call(f"OM({n},{m}) B={B} engine={engine_sel} staged={staged}", B, outs, want, cnt)

    def issue(e, s):
        o = dict(d_decisions=outs["decisions"].data_ptr(), d_outcome=outs["outcome"].data_ptr(),
                 d_counters=c.cnt.data_ptr(), stream=s)
        if staged:
            ins = dict(d_faulty=outs["faulty"].data_ptr(), d_order=outs["order"].data_ptr())
            e.gen_inputs_device(L.make_params(n, m, **kw), B, stream=s, **ins)
            e.run_device(L.make_params(n, m, seed=kw["seed"], first_trial=first, engine=engine_sel), B, **ins, **o)
        else:
            e.run_device(L.make_params(n, m, engine=engine_sel, **kw), B, **o)
    c.issue = issue
    return c


def table_call(n, B):
    """ba_mt_table_device + ba_run_trials_device(BA_LIE_TABLE) on one stream: config 1."""
    import torch
    from ba_amd import lib as L
    seeds, faulty, order, want, cnt = ref_table(n, B)
    stride = L.table_stride(n)
    d_s = torch.from_numpy(seeds.view(np.int64)).cuda()
    d_f = torch.from_numpy(faulty.view(np.int32)).cuda()
    d_o = torch.from_numpy(order).cuda()
    outs = _bufs(B)
    outs["table"] = torch.empty((B, stride), dtype=torch.int32, device="cuda")
    c = Call(f"table mode n={n} B={B}", B, outs, want, cnt)
    c.keep = (d_s, d_f, d_o)

    def issue(e, s):
        e.mt_table_device(n, 1, B, d_s.data_ptr(), d_f.data_ptr(), stride, outs["table"].data_ptr(), stream=s)
        e.run_device(L.make_params(n, 1, lie_mode=L.LIE_TABLE, stride=stride), B, d_faulty=d_f.data_ptr(),
                     d_order=d_o.data_ptr(), d_table=outs["table"].data_ptr(),
                     d_decisions=outs["decisions"].data_ptr(), d_outcome=outs["outcome"].data_ptr(),
                     d_counters=c.cnt.data_ptr(), stream=s)
    c.issue = issue
    return c


def sm_call(n, m, B, first=FIRST, ref=True):
    import torch
    from ba_amd import lib as L
    outs = _bufs(B, vsets=torch.int64)
    c = Call(f"SM({n},{m}) B={B}", B, outs, *(ref_sm(n, m, B, first) if ref else (None, None)))
    c.issue = lambda e, s: e.run_sm_device(
        L.make_params(n, m, **model_kw(n, first)), B, d_decisions=outs["decisions"].data_ptr(),
        d_outcome=outs["outcome"].data_ptr(), d_vsets=outs["vsets"].data_ptr(), d_counters=c.cnt.data_ptr(),
        stream=s)
    return c


def adv_call(n, m, policy, B, first=FIRST):
    from ba_amd import lib as L
    outs = _bufs(B)
    c = Call(f"ADV({n},{m}) policy={policy} B={B}", B, outs, *ref_adv(n, m, policy, B, first))
    c.issue = lambda e, s: e.run_adv_device(
        L.make_params(n, m, **model_kw(n, first)), B, policy, d_decisions=outs["decisions"].data_ptr(),
        d_outcome=outs["outcome"].data_ptr(), d_counters=c.cnt.data_ptr(), stream=s)
    return c


def king_call(kind, n, m, policy, B, first=FIRST, ref=True):
    import torch
    from ba_amd import lib as L
    outs = _bufs(B, settled=torch.uint8)
    c = Call(f"{kind}({n},{m}) policy={policy} B={B}", B, outs,
             *(ref_king(kind, n, m, policy, B, first) if ref else (None, None)))

    def issue(e, s):
        run = e.run_king_device if kind == "king" else e.run_king3_device
        run(L.make_params(n, m, **model_kw(n, first)), B, policy, d_decisions=outs["decisions"].data_ptr(),
            d_outcome=outs["outcome"].data_ptr(), d_settled=outs["settled"].data_ptr(),
            d_counters=c.cnt.data_ptr(), stream=s)
    c.issue = issue
    return c


# --- capture, replay three times ----------------------------------------------------------
def eager(eng, call, stream, times, what):
    import torch
    with torch.cuda.stream(stream):
        call.poison()
        call.cnt.zero_()
        for _ in range(times):
            call.issue(eng, stream.cuda_stream)
    torch.cuda.synchronize()
    call.verify(times, what)


def capture(eng, call, stream, zero_in_graph):
    """The eager warm-up, then the identical call captured (ba.h's capture contract)."""
    import torch
    eager(eng, call, stream, 1, "warm-up")
    with torch.cuda.stream(stream):
        call.cnt.zero_()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=stream):
        if zero_in_graph:
            call.cnt.zero_()
        call.issue(eng, stream.cuda_stream)
    return g


def replay(g, call, stream):
    import torch
    with torch.cuda.stream(stream):
        call.poison()
        g.replay()


def graph_rounds(make_call, between=None):
    """Both variants of a case, each on an Engine of its own: d_counters left alone
    (after replay k: k x the reference) and zeroed inside the graph (the reference each
    time); outputs poisoned before and exact after each of three replays; `between`: an
    eager call of another entry on the same ctx after replay 2; at the end the captured
    call once more eagerly (the replays left the sink zero)."""
    import torch
    from ba_amd import lib as L
    for zero_in_graph in (False, True):
        eng = L.Engine(0)
        try:
            call = make_call()
            s = torch.cuda.Stream()
            s.wait_stream(torch.cuda.current_stream())
            g = capture(eng, call, s, zero_in_graph)
            for k in (1, 2, 3):
                replay(g, call, s)
                torch.cuda.synchronize()
                call.verify(1 if zero_in_graph else k, f"zero_in_graph={zero_in_graph} replay {k}")
                if k == 2 and between is not None:
                    scratch = eng.memory()["scratch"]
                    eager(eng, between(), s, 1, "eager call between replays")
                    assert eng.memory()["scratch"] == scratch  # a graph's buffers stay valid
            eager(eng, call, s, 1, f"zero_in_graph={zero_in_graph} eager after replays")
            del g
        finally:
            torch.cuda.synchronize()
            eng.close()


@pytest.mark.parametrize("B", [B_OM3, B_OM3_REP])
def test_graph_om3wt_drawn(B):
    """(10, 3) AUTO, drawn inputs.  71 tasks are 18 reporting blocks, which add straight
    into d_counters; 261 tasks are 66, which go through the sink's replicas.  Between
    replays 2 and 3 the ctx makes an eager SM call."""
    shape = wave_shape(8, B, None, cu_count(), OM3W_BPC)
    assert (shape.blocks > 64) == (B == B_OM3_REP), shape
    graph_rounds(lambda: om_call(10, 3, B), between=lambda: sm_call(4, 1, 229))


def test_graph_om3wt_staged():
    """ba_gen_inputs_device + the GIVEN run in ONE graph (bench.py's staging); the staged
    inputs are poisoned and checked too."""
    graph_rounds(lambda: om_call(10, 3, B_OM3, staged=True))


def test_graph_om4w_task_counter(monkeypatch):
    """(9, 4) under BA_WAVE_MAX_BLOCKS=2: 12 tasks on 8 waves, handed out by the ctx's task
    counter, which launch_wave zeroes on the launch's stream.  The zeroing must be a node
    of the graph: a replay that started from the previous replay's count would find no
    task left after the first wave-round."""
    monkeypatch.setenv("BA_WAVE_MAX_BLOCKS", "2")
    monkeypatch.setenv("BA_WAVE_STATIC_TASKS", "0")
    monkeypatch.delenv("BA_FUSED_KIND", raising=False)
    W = om4w_words(9)
    shape = wave_shape(W, B_OM4, "2", cu_count())
    assert W == 10 and shape.persistent and (shape.tasks, shape.blocks) == (12, 2), shape
    graph_rounds(lambda: om_call(9, 4, B_OM4))


@pytest.mark.parametrize("n,m,engine_sel", [(16, 2, 2), (7, 2, 0)])
def test_graph_scratch_engines(monkeypatch, n, m, engine_sel):
    """(16, 2) on ENGINE_LEVELS (depth 2: the multi-launch pipeline, no cascade) and
    (7, 2), the block kernel k_fused: the launches of a replay read and write the ctx's
    scratch and partial rows at the addresses the capture saw."""
    from ba_amd import lib as L
    for k in ("BA_FUSED_KIND", "BA_SCRATCH_BYTES", "BA_NO_CASCADE"):
        monkeypatch.delenv(k, raising=False)
    assert engine_sel == L.ENGINE_LEVELS or L.load().ba_engine_for(n, m) == L.ENGINE_FUSED
    graph_rounds(lambda: om_call(n, m, B_LEV, engine_sel=engine_sel))


def test_graph_table_mode():
    """ba_mt_table_device + ba_run_trials_device(BA_LIE_TABLE) in one graph (config 1); the
    table itself is poisoned and checked against ba_mt_table."""
    graph_rounds(lambda: table_call(4, B69))


def test_graph_sm():
    assert wave_units(B69) > 64
    graph_rounds(lambda: sm_call(10, 3, B69))


@pytest.mark.parametrize("policy", [A.SPLIT, A.ANTI])
@pytest.mark.parametrize("B", [B69, 64 * 512 + 37])
def test_graph_adv(policy, B):
    """(7, 2): a k_adv block takes 32 words, so 69 words are 12 reporting waves (straight
    into d_counters) and 513 words are 68 (the sink's replicas)."""
    assert adv_units(7, B) == (12 if B == B69 else 68)
    graph_rounds(lambda: adv_call(7, 2, policy, B))


def test_graph_king():
    assert wave_units(B69) > 64
    graph_rounds(lambda: king_call("king", 9, 2, K.KING_COIN, B69))


@pytest.mark.parametrize("n,m,policy", [(10, 3, K3.KING_COIN), (4, 1, K3.KING_SPLIT)])
def test_graph_king3(n, m, policy):
    """Between replays 2 and 3 the ctx makes an eager OM call."""
    assert wave_units(B69) > 64
    graph_rounds(lambda: king_call("king3", n, m, policy, B69), between=lambda: om_call(10, 3, 777))


def test_two_ctxs_two_graphs_alternate():
    """The k_om3wt graph and the SM graph, each from its own ctx, replayed alternately on
    two streams for three rounds with no host sync in between: after one final sync every
    output is exact and the counters, never zeroed, are 3 x the reference."""
    import torch
    from ba_amd import lib as L
    engs = [L.Engine(0), L.Engine(0)]
    try:
        calls = [om_call(10, 3, B_OM3_REP), sm_call(10, 3, B69)]
        sts = [torch.cuda.Stream(), torch.cuda.Stream()]
        for s in sts:
            s.wait_stream(torch.cuda.current_stream())
        gs = [capture(e, c, s, False) for e, c, s in zip(engs, calls, sts)]
        for _ in range(3):
            for g, c, s in zip(gs, calls, sts):
                replay(g, c, s)
        torch.cuda.synchronize()
        for c in calls:
            c.verify(3, "after three alternating rounds")
        del gs
    finally:
        torch.cuda.synchronize()
        for e in engs:
            e.close()


# --- the two refusals -----------------------------------------------------------------------
ENUM_CASE = (5, 2, 0b00110, O.RETREAT)  # 12 free bits, violations from strategy 15 on


def test_enum_device_is_refused_under_capture():
    """ba_enum_run_device copies its slot map from host memory that dies with the call, so
    on a capturing stream it returns BA_ENOTSUP before it touches the stream: the capture,
    which also holds an SM call, ends valid and replays exactly, and the same enum call
    made eagerly afterwards is exact."""
    import torch
    from ba_amd import lib as L
    n, m, F, o = ENUM_CASE
    count = 1 << E.bits_formula(n, m, F)
    want, cnt, wit = ref_enum(n, m, F, o, 0, count)
    en = Call("enum", count, _bufs(count), want, cnt)
    d_wit = torch.full((1,), -1, dtype=torch.int64, device="cuda")
    en.issue = lambda e, s: e.run_enum_device(
        L.make_params(n, m), F, o, count, d_decisions=en.outs["decisions"].data_ptr(),
        d_outcome=en.outs["outcome"].data_ptr(), d_counters=en.cnt.data_ptr(), d_witness=d_wit.data_ptr(),
        stream=s)
    eng = L.Engine(0)
    try:
        sm = sm_call(10, 3, B69)
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        eager(eng, sm, s, 1, "warm-up")
        eager(eng, en, s, 1, "enum warm-up")
        with torch.cuda.stream(s):
            sm.cnt.zero_()
            en.poison()
            en.cnt.zero_()
            d_wit.fill_(-1)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            sm.issue(eng, s.cuda_stream)
            with pytest.raises(L.BAError) as ei:
                en.issue(eng, s.cuda_stream)
            assert ei.value.code == L.ENOTSUP and "captur" in str(ei.value)
        for k in (1, 2, 3):
            replay(g, sm, s)
            torch.cuda.synchronize()
            sm.verify(k, f"replay {k}")
        # the refused call queued nothing: its buffers are as they were
        got, c = en.read()
        assert all(int(x) == 2**64 - 1 for x in got["decisions"][:64]) and set(got["outcome"].tolist()) == {254}
        assert c == [0] * 16 and int(d_wit.cpu().numpy().view(np.uint64)[0]) == 2**64 - 1
        eager(eng, en, s, 1, "eager enum after the capture")
        assert int(d_wit.cpu().numpy().view(np.uint64)[0]) == wit == 15
        del g
    finally:
        torch.cuda.synchronize()
        eng.close()


def test_profile_skips_capturing_streams(monkeypatch):
    """With profiling on, launches on a capturing stream are not bracketed by events (an
    event recorded there is a graph node, never recorded eagerly, and ba_profile_read could
    not synchronise on it): after the warm-up, the capture and three replays the profile
    is exactly the warm-up's kernels, one launch each, and the replays are exact."""
    import torch
    from ba_amd import lib as L
    for k in ("BA_OM3W_TABLE", "BA_FUSED_KIND", "BA_WAVE_MAX_BLOCKS"):
        monkeypatch.delenv(k, raising=False)
    eng = L.Engine(0)
    try:
        call = om_call(10, 3, B_OM3, staged=True)
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        eng.profile(True)
        g = capture(eng, call, s, True)
        for k in (1, 2, 3):
            replay(g, call, s)
            torch.cuda.synchronize()
            call.verify(1, f"replay {k}")
        prof = {k: v[0] for k, v in eng.profile_read().items()}
        assert set(prof) == {"k_gen_inputs", "k_om3wt"} and set(prof.values()) == {1}, prof
        assert eng.lib.ba_profile_read(eng.handle, 0, None, 0, None, None) == L.OK
        eng.profile(False)
        del g
    finally:
        torch.cuda.synchronize()
        eng.close()


# --- one ctx, two streams, every entry ---------------------------------------------------------
HEAD = 4389      # trials of a 2^18-trial call that are compared with its model ...
HEAD_N32 = 229   # ... and at n = 32, where the models take 12 ms (KING3) and 2 ms (KING) a trial


def test_one_ctx_two_streams_every_entry(engine):
    """Seven calls of ONE ctx issued back to back, alternating over two streams, with no
    host sync: KING3 COIN (32, 10) on 2^18 trials first -- the long call (about 180 us by
    the README's 715 us per 1M trials: inferred, not measured here), so that the next is
    submitted while it runs -- then OM (10, 3), SM (10, 3) on 2^18, ADV ANTI (7, 2), KING
    SPLIT (32, 7) on 2^18, ENUM (7, 2) on 2^20 strategies (its slot map lands in the shared
    scratch) and the staged LEVELS (16, 2) run, which uses the scratch too.  The calls of
    at most 36k trials are compared whole with the oracle or their model.  The 2^18-trial
    calls and the enum call: their first trials with the model (trials are keyed by global
    index; 4389 of them, 229 at n = 32 where 4389 would take the KING3 model 53 s and the
    KING model 9 s), and the whole output and the counters with the same call made alone,
    between host syncs, on a fresh ctx.

    What this test cannot show is that it would fail without the ctx's ordering
    (ctx_order / ctx_mark): calls that share only the sink and do not overlap in time
    would pass without it, and nothing here forces an overlap."""
    import torch
    from ba_amd import lib as L
    T = 1 << 18
    n_e, m_e, F_e, o_e, T_e = 7, 2, 0b0000110, O.ATTACK, 1 << 20

    def enum_call():
        c = Call("ENUM(7,2)", T_e, _bufs(T_e))
        c.wit = torch.full((1,), -1, dtype=torch.int64, device="cuda")
        c.outs["witness"] = c.wit
        c.issue = lambda e, s: e.run_enum_device(
            L.make_params(n_e, m_e), F_e, o_e, T_e, d_decisions=c.outs["decisions"].data_ptr(),
            d_outcome=c.outs["outcome"].data_ptr(), d_counters=c.cnt.data_ptr(), d_witness=c.wit.data_ptr(),
            stream=s)
        return c

    big = {0: (king_call("king3", 32, 10, K3.KING_COIN, T, ref=False), HEAD_N32,
               lambda h: ref_king("king3", 32, 10, K3.KING_COIN, h)[0]),
           2: (sm_call(10, 3, T, ref=False), HEAD, lambda h: ref_sm(10, 3, h)[0]),
           4: (king_call("king", 32, 7, K.KING_SPLIT, T, ref=False), HEAD_N32,
               lambda h: ref_king("king", 32, 7, K.KING_SPLIT, h)[0]),
           5: (enum_call(), HEAD, lambda h: ref_enum(n_e, m_e, F_e, o_e, 0, h)[0])}
    calls = {1: om_call(10, 3, B_OM3), 3: adv_call(7, 2, A.ANTI, B69),
             6: om_call(16, 2, B_LEV, engine_sel=L.ENGINE_LEVELS, staged=True)}
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    for s in (s1, s2):
        s.wait_stream(torch.cuda.current_stream())
    # the big calls alone, each on a fresh ctx between host syncs: head against the model
    for i, (c, head, model) in big.items():
        solo = L.Engine(0)
        try:
            with torch.cuda.stream(s1):
                c.poison()
                c.issue(solo, s1.cuda_stream)
            torch.cuda.synchronize()
        finally:
            solo.close()
        got, _ = c.read()
        for k, want in model(head).items():
            same(got[k][:head], want, f"{c.name} alone, first {head} trials vs the model: {k}")
        c.adopt()
        assert c.ref_cnt[0] == c.B, c.name
        calls[i] = c
    order = [calls[i] for i in range(7)]
    for c in order:
        c.poison()
        c.cnt.zero_()
    torch.cuda.synchronize()
    for i, c in enumerate(order):  # back to back, no host sync (the enum entry itself waits: ba.h)
        c.issue(engine, (s1, s2)[i % 2].cuda_stream)
    torch.cuda.synchronize()
    for c in order:
        c.verify(1, "one ctx, two streams")
