"""The 64-bit global trial index on every engine (docs/SEMANTICS.md §3-§4).

Every coin is keyed by the global trial index t: the lie stream by the trial
word w = t // 64 (Philox ctr words 2, 3 = w_lo, w_hi), the synthetic inputs by t
itself (ctr words 2, 3 = t_lo, t_hi).  Each kernel family forms those counter
words at its own sites; here every one of them runs with a non-zero upper word
and with a launch in which the lower word carries into the upper one, bit-exact
against the oracle on decisions, outcome bytes and all 12 counters -- once with
inputs drawn in the kernel and once with staged inputs (ba_gen_inputs_device,
then GIVEN mode), and with the profile showing that the kernel meant ran.
"""
import ctypes
import functools

import numpy as np
import pytest

import ba_oracle as O
import oracle_c
import sm_model as S
from test_gpu import same
from test_gpu_om3w_table import check_case
from test_gpu_om3w_trim import run_staged, task_words
from test_gpu_sm import check as check_sm

pytestmark = pytest.mark.gpu


# --- the start points ---------------------------------------------------------------
def T32(a):
    """The input stream's ctr word 2 carries into word 3 `a` words into the launch."""
    return 2**32 - 64 * a


def W32(a):
    """The lie stream's ctr word 2 carries into word 3 `a` words into the launch."""
    return 2**38 - 64 * a


HI = 64 * (0x03FFFFFF * 2**32 + 9)  # the largest w_hi (t_hi = 0xFFFFFFC0), no straddle


def TOP(B):
    """The run ends exactly at 2^64."""
    assert B % 64 == 0
    return 2**64 - B


STARTS1 = {"W32": W32(1), "T32": T32(1), "HI": HI}  # block kernels: one word below, the rest above


def task_starts(W):
    """Per-wave task kernels (W words per task): the boundary inside a task
    (a = W + 2) and on a task edge (a = W), both streams, and HI."""
    return {"W32in": W32(W + 2), "W32edge": W32(W), "T32in": T32(W + 2), "T32edge": T32(W), "HI": HI}


@functools.lru_cache(maxsize=None)
def lie_sensitive_seed(n, m, first):
    """A seed for a ONE-trial case that hangs on the upper half of its trial word: the
    first under which the oracle's decisions for trial `first` (inputs drawn with up
    to n faulty generals) change when the same inputs are run at the trial word with
    that half cleared.  OM(m) is indifferent to the lies of most single trials (few
    traitors: the guarantee holds; nearly all: the majorities collapse to retreat);
    such a trial would pass whatever the kernel did with the word's upper half."""
    low = ((first >> 6) & 0xFFFFFFFF) << 6
    for seed in range(0x64B17, 0x64B17 + 256):
        fm, oc = O.gen(n, seed, O.FAULTY_RANDOM, n, O.ORDER_RANDOM, 1, first)
        d = [oracle_c.run(n, m, 1, seed=seed, faulty=[fm], order=[oc], first_trial=t)[0][0] for t in (first, low)]
        if d[0] != d[1]:
            return seed
    raise AssertionError("no seed found")


def kw_for(n, first, single_m=None):
    """In-kernel draws: up to (n-1)//3 + 2 faulty generals of n (above the bound,
    so faulty senders -- and their lies -- are common), random orders.  `single_m`
    (batch 1 at depth m): up to n, under lie_sensitive_seed."""
    from ba_amd import lib as L
    if single_m is not None:
        return dict(seed=lie_sensitive_seed(n, single_m, first), faulty_mode=L.FAULTY_RANDOM, f=n,
                    order_mode=L.ORDER_RANDOM, first_trial=first)
    return dict(seed=0x64B17 + n, faulty_mode=L.FAULTY_RANDOM, f=min(n, (n - 1) // 3 + 2),
                order_mode=L.ORDER_RANDOM, first_trial=first)


@functools.lru_cache(maxsize=None)
def oracle(n, m, B, first):
    """oracle_c.run of a case (computed once; the switch variants share it)."""
    return oracle_c.run(n, m, B, **kw_for(n, first, m if B == 1 else None))


@functools.lru_cache(maxsize=None)
def oracle_votes(n, m, B, first, level):
    return (oracle_c.votes if level == 1 else oracle_c.votes2)(n, m, B, **kw_for(n, first))


def env(monkeypatch, **kv):
    for k, v in kv.items():
        if v is None:
            monkeypatch.delenv(k, raising=False)
        else:
            monkeypatch.setenv(k, str(v))


def staged_inputs(e, n, m, B, kw):
    """ba_gen_inputs_device buffers read back to the host; they are the oracle's."""
    import torch
    from ba_amd import lib as L
    fb = torch.empty(B, dtype=torch.int32, device="cuda")
    ob = torch.empty(B, dtype=torch.uint8, device="cuda")
    e.gen_inputs_device(L.make_params(n, m, **kw), B, d_faulty=fb.data_ptr(), d_order=ob.data_ptr(),
                        stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    fm, oc = fb.cpu().numpy().view(np.uint32), ob.cpu().numpy()
    gf, go = oracle_c.sliced_gen(n, B, seed=kw["seed"], faulty_mode=kw["faulty_mode"], f=kw["f"],
                                 order_mode=kw["order_mode"], first_trial=kw["first_trial"])
    same(fm, gf, "staged faulty sets")
    same(oc, go, "staged orders")
    return fm, oc


def check(n, m, B, first, tag, engine=0):
    """One case on a fresh ctx, drawn then staged, against the oracle.  Returns the
    profiles {kernel: launches} of the drawn and of the staged run.  AUTO engine:
    the staged run is the device path of run_staged; a forced engine takes the
    staged buffers through the host entry (run_staged's params are AUTO)."""
    from ba_amd import lib as L
    kw = kw_for(n, first, m if B == 1 else None)
    od, oo, ocnt = oracle(n, m, B, first)
    e = L.Engine(0)
    try:
        e.profile(True)
        res = e.run(n, m, B, engine=engine, **kw)
        prof_d = {k: v[0] for k, v in e.profile_read().items()}
        same(res.decisions, od, "decisions, drawn " + tag)
        same(res.outcome, oo, "outcome, drawn " + tag)
        assert {k: res.counters[k] for k in ocnt} == ocnt, "drawn " + tag
        e.profile(True)
        if engine == L.ENGINE_AUTO:
            dec, out, cnt = run_staged(e, n, m, B, kw)
            prof_s = {k: v[0] for k, v in e.profile_read().items() if k != "k_gen_inputs"}
        else:
            fm, oc = staged_inputs(e, n, m, B, kw)
            e.profile(True)
            r = e.run(n, m, B, seed=kw["seed"], first_trial=first, faulty=fm, order=oc, engine=engine)
            prof_s = {k: v[0] for k, v in e.profile_read().items()}
            dec, out, cnt = r.decisions, r.outcome, [r.counters[k] for k in ocnt]
        same(dec, od, "decisions, staged " + tag)
        same(out, oo, "outcome, staged " + tag)
        assert cnt == list(ocnt.values()), "staged " + tag
    finally:
        e.close()
    return prof_d, prof_s


# --- WAVE depth 3: k_om3w (n != 10), k_om3wt / k_om3w at n = 10 ---------------------------
@pytest.mark.parametrize("cap", [None, "1"])
@pytest.mark.parametrize("start", ["W32in", "W32edge", "T32in", "T32edge", "HI"])
@pytest.mark.parametrize("n", [5, 14])  # Om3W<N>::W = 21 and 5: the widest and narrowest task
def test_om3w(monkeypatch, n, start, cap):
    """The default grid, and one block walking every task (BA_WAVE_MAX_BLOCKS=1)."""
    W = task_words(n)
    first = task_starts(W)[start]
    env(monkeypatch, BA_OM3W_TABLE=None, BA_FUSED_KIND=None, BA_WAVE_MAX_BLOCKS=cap)
    check_case(n, 64 * W * 5 + 37, kw_for(n, first), "k_om3w", f"n={n} {start} cap={cap}")


@pytest.mark.parametrize("cap", [None, "1"])
@pytest.mark.parametrize("start", ["T32in", "T32edge", "HI"])
def test_om3wt_n10(monkeypatch, start, cap):
    """n = 10 (W32 is in test_gpu_om3w_table.py): the trial words of these starts
    share one upper half, so the pair-table kernel runs."""
    first = task_starts(8)[start]
    env(monkeypatch, BA_OM3W_TABLE=None, BA_FUSED_KIND=None, BA_WAVE_MAX_BLOCKS=cap)
    check_case(10, 64 * 8 * 3 + 37, kw_for(10, first), "k_om3wt", f"n=10 {start} cap={cap}")


@pytest.mark.parametrize("cap", [None, "1"])
def test_om3w_n10_ends_at_2_64(monkeypatch, cap):
    """Two whole tasks that end exactly at trial 2^64 (either n = 10 kernel may run)."""
    env(monkeypatch, BA_OM3W_TABLE=None, BA_FUSED_KIND=None, BA_WAVE_MAX_BLOCKS=cap)
    B = 64 * 8 * 2
    prof, _ = check(10, 3, B, TOP(B), f"n=10 TOP cap={cap}")
    assert any(k.startswith("k_om3w") for k in prof), prof


# --- WAVE depth 4: k_om4w -----------------------------------------------------------------
def loop_starts(W):
    """k_om4w's task loop under BA_WAVE_MAX_BLOCKS=1 (4 waves, 10 tasks): the boundary
    inside task 8 (a = 9 W - 2 words into the launch) and on its edge (a = 8 W), both
    streams.  Task 8 is of the third wave-round: a wave reaches it through the loop."""
    return {"W32loop_in": W32(9 * W - 2), "W32loop_edge": W32(8 * W), "T32loop_in": T32(9 * W - 2),
            "T32loop_edge": T32(8 * W)}


@pytest.mark.parametrize("static", ["0", "1"])
@pytest.mark.parametrize("start", ["W32in", "W32edge", "T32in", "T32edge", "HI", "W32loop_in", "W32loop_edge",
                                   "T32loop_in", "T32loop_edge"])
@pytest.mark.parametrize("n", [6, 13])  # Om4W<N>::W = 64 // (n - 3) = 21 and 6
def test_om4w(monkeypatch, n, start, static):
    """The default grid (4 tasks on 4 waves: no task loop, whatever `static`), and, the
    *loop* starts, one block walking 10 tasks (BA_WAVE_MAX_BLOCKS=1) with the carry in a
    task of the third wave-round: fetched from the ctx's dynamic task counter, or
    reached by the static stride (BA_WAVE_STATIC_TASKS=1).  The staged run of each is
    k_om4w<N, true>."""
    from wave_shape import om4w_words, wave_shape
    W = om4w_words(n)
    assert W == 64 // (n - 3)
    loop = start in loop_starts(W)
    if loop:
        first, B, cap = loop_starts(W)[start], 64 * W * 9 + 11, "1"
        shape = wave_shape(W, B, cap)
        assert shape.persistent and (shape.tasks, shape.blocks) == (10, 1), shape
        # the word in which the counter word carries lies in task 8 or later (round 3)
        carry_word = ((2**38 if start.startswith("W32") else 2**32) - first) // 64
        assert 8 * W <= carry_word < shape.words and carry_word // W >= 2 * 4 * shape.blocks
    else:
        first, B, cap = task_starts(W)[start], 64 * W * 3 + 11, None
        shape = wave_shape(W, B, cap)
        assert not shape.persistent and shape.tasks == 4, shape
    env(monkeypatch, BA_FUSED_KIND=None, BA_WAVE_MAX_BLOCKS=cap, BA_WAVE_STATIC_TASKS=static)
    for prof in check(n, 4, B, first, f"n={n} {start} static={static}"):
        assert prof.get("k_om4w") == 1 and "k_fused" not in prof, prof


# --- the generic FUSED block kernel k_fused ----------------------------------------------
@pytest.mark.parametrize("start", list(STARTS1))
@pytest.mark.parametrize("n,m,kind", [(7, 3, "2"), (7, 4, "2"), (7, 2, None)])
def test_fused_block_kernel(monkeypatch, n, m, kind, start):
    """BA_FUSED_KIND=2 on a depth-3 and a depth-4 tree (instead of the WAVE kernels),
    and (7, 2), which takes k_fused by default."""
    from ba_amd import lib as L
    assert L.load().ba_engine_for(n, m) == L.ENGINE_FUSED
    env(monkeypatch, BA_FUSED_KIND=kind)
    for prof in check(n, m, 64 * 3 + 9, STARTS1[start], f"n={n} m={m} kind={kind} {start}"):
        assert prof.get("k_fused") == 1 and not any(k.startswith("k_om") for k in prof), prof


# --- LEVELS, the multi-launch pipeline ------------------------------------------------------
LEVELS_SWITCHES = ["BA_NO_INPUT_FUSION", "BA_NO_TOP_RELAY", "BA_NO_LEAF_UP", "BA_NO_TAIL",
                   "BA_NO_LEAF_FUSION"]
LEVELS_VARIANTS = ["default"] + LEVELS_SWITCHES + ["chunks", "chunks+BA_NO_INPUT_FUSION"]


def levels_env(monkeypatch, switch=None, budget=None):
    env(monkeypatch, BA_NO_CASCADE="1", BA_SCRATCH_BYTES=budget, **{k: None for k in LEVELS_SWITCHES})
    if switch:
        monkeypatch.setenv(switch, "1")


@functools.lru_cache(maxsize=None)
def levels_scratch_bytes(n, m, B):
    """Scratch the multi-launch pipeline holds after a batch run as ONE chunk
    (ba_ctx_memory; the default budget): its bytes per 64-trial word times the words."""
    from ba_amd import lib as L
    e = L.Engine(0)
    try:
        e.run(n, m, B, engine=L.ENGINE_LEVELS, **kw_for(n, 0))
        return e.memory()["scratch"]
    finally:
        e.close()


@pytest.mark.parametrize("variant", LEVELS_VARIANTS)
@pytest.mark.parametrize("start", list(STARTS1))
@pytest.mark.parametrize("n,m,B", [(7, 2, 64 * 5 + 9), (10, 3, 64 * 5 + 9), (16, 5, 130)])
def test_levels_pipeline(monkeypatch, n, m, B, start, variant):
    """k_input / k_relay_top / k_relay / k_leaf / k_leaf_up / k_majority / k_tail /
    k_epilogue (BA_NO_CASCADE=1 keeps (10, 3) and (16, 5) off k_cascade): the default
    fusions, each fusion switched off alone, and a scratch budget of two words per
    chunk -- three chunks at six words, the boundary in the middle of the first, each
    chunk keyed by first_trial + trial0 and small enough for the inputs fused into
    k_relay_top; the same with BA_NO_INPUT_FUSION, which then changes the launches.
    (The three words of (16, 5) make two such chunks: a third would need an edge on
    the boundary.)"""
    from ba_amd import lib as L
    words = (B + 63) // 64
    chunks, _, switch = variant.partition("+")
    if not chunks.startswith("chunks"):
        chunks, switch = "", variant if variant != "default" else ""
    budget = None
    if chunks:
        levels_env(monkeypatch)
        budget = levels_scratch_bytes(n, m, B) * 5 // (2 * words)  # 2.5 words' worth
    levels_env(monkeypatch, switch or None, budget)
    me = L.effective_depth(n, m)
    for prof in check(n, m, B, STARTS1[start], f"n={n} m={m} {start} {variant}", engine=L.ENGINE_LEVELS):
        assert not any(k.startswith(("k_cascade", "k_om", "k_fused")) for k in prof), prof
        leafk = [k for k in prof if k.startswith("k_leaf")]
        if switch == "BA_NO_LEAF_FUSION":
            assert not leafk and "k_relay_leaf" in prof, prof
        elif switch == "BA_NO_LEAF_UP" or me < 3:
            assert leafk == ["k_leaf"], prof
        else:
            assert leafk == ["k_leaf_up"], prof
        assert ("k_relay_top" in prof) == (switch != "BA_NO_TOP_RELAY"), prof
        if switch == "BA_NO_TOP_RELAY":
            assert "k_relay_inner" in prof, prof
        if switch == "BA_NO_TAIL":
            assert "k_tail" not in prof and "k_epilogue" in prof, prof
        if chunks:
            assert prof[leafk[0]] == (words + 1) // 2, prof  # chunks of two words
            assert ("k_input" in prof) == (switch == "BA_NO_INPUT_FUSION"), prof


# --- k_cascade ----------------------------------------------------------------------------
CASC_PATHS = {"co": dict(BA_CASC_CO="1", BA_CASC_TWO=None, BA_CASC_CHECK=None),
              "two": dict(BA_CASC_CO="0", BA_CASC_TWO="1", BA_CASC_CHECK=None),
              "check": dict(BA_CASC_CO=None, BA_CASC_TWO=None, BA_CASC_CHECK="1")}
CASC_STARTS = {"W32": (W32(1), 130), "T32": (T32(1), 130), "at2p38": (2**38, 1), "HI": (HI, 1)}


CASC_CHECK_SHAPES = [(8, 5), (16, 5)]  # ba_cascade.hip BA_CASC_CHECK_SHAPES (not (16, 4))
CASC_CASES = [(n, m, start, path) for n, m in [(8, 5), (16, 4), (16, 5)] for start in CASC_STARTS
              for path in CASC_PATHS if path != "check" or (n, m) in CASC_CHECK_SHAPES]


@pytest.mark.parametrize("n,m,start,path", CASC_CASES)
def test_cascade(monkeypatch, n, m, start, path):
    """The one-launch CO path, the two-launch path and the check build (the shapes
    that have one).  That the check build is what ran shows in its own counter, as in
    test_gpu_cascade.py: the same call leaves BA_C_CHECK_MISMATCH at 0, and at exactly
    1 with one stale tag injected (BA_CASC_CHECK=2); the plain build leaves both at 0."""
    import torch
    from ba_amd import lib as L
    first, B = CASC_STARTS[start]
    env(monkeypatch, BA_NO_CASCADE=None, BA_SCRATCH_BYTES=None, BA_CASC_LAT=None, BA_CASC_WTOP=None,
        BA_CASC_MTOP=None, **{k: None for k in LEVELS_SWITCHES})
    env(monkeypatch, **CASC_PATHS[path])
    for prof in check(n, m, B, first, f"n={n} m={m} {start} {path}", engine=L.ENGINE_LEVELS):
        assert any(k.startswith("k_cascade") for k in prof), prof
        assert not any(k.startswith(("k_leaf", "k_relay", "k_majority", "k_om", "k_fused")) for k in prof), prof
        if path == "co":
            assert "k_cascade_co" in prof, prof
        if path == "two":
            assert "k_cascade_co" not in prof, prof
            assert any(k in prof for k in ("k_cascade_top", "k_cascade_wtop", "k_cascade_mtop")), prof
    if path == "check":
        kw = kw_for(n, first, m if B == 1 else None)
        cnt = torch.zeros((2, 16), dtype=torch.int64, device="cuda")
        e = L.Engine(0)
        try:
            for i, mode in enumerate(("1", "2")):
                monkeypatch.setenv("BA_CASC_CHECK", mode)
                e.run_device(L.make_params(n, m, engine=L.ENGINE_LEVELS, **kw), B, d_counters=cnt[i].data_ptr(),
                             stream=torch.cuda.current_stream().cuda_stream)
            torch.cuda.synchronize()
        finally:
            e.close()
        got = cnt.cpu().tolist()
        assert [row[14] for row in got] == [0, 1], got  # BA_C_CHECK_MISMATCH
        assert got[0][:12] == list(oracle(n, m, B, first)[2].values())


# --- the split-vote entries -----------------------------------------------------------------
@pytest.mark.parametrize("nocasc", ["0", "1"])
@pytest.mark.parametrize("level", [1, 2])
@pytest.mark.parametrize("n,m,ub,start", [(9, 4, 3, "W32"), (9, 4, 3, "T32"), (9, 4, 3, "HI"),
                                          (16, 5, 7, "W32")])
def test_split_votes(monkeypatch, n, m, ub, start, level, nocasc):
    """ba_subtree_votes_device / ba_split_votes_device over a range of two subtrees,
    then over every unit, against the oracle's votes; ba_root_from_votes_device /
    ba_root_from_split_votes_device over those rows against oracle_c.run.  Through
    the cascade's range mode and through the LEVELS kernels (BA_NO_CASCADE=1)."""
    import torch
    from ba_amd import lib as L
    env(monkeypatch, BA_NO_CASCADE=nocasc, BA_CASC_CO=None, BA_CASC_TWO=None, BA_CASC_CHECK=None,
        BA_SCRATCH_BYTES=None, **{k: None for k in LEVELS_SWITCHES})
    B, first = 130, STARTS1[start]
    kw = kw_for(n, first)
    od, oo, ocnt = oracle(n, m, B, first)
    v_or = oracle_votes(n, m, B, first, level)
    units, per, W = L.split_units(n, m, level), n - 1 - level, (B + 63) // 64
    ub = ub if level == 1 else ub * 2 - 1  # level 2: an odd unit, mid first-hop subtree
    s = torch.cuda.current_stream().cuda_stream
    e = L.Engine(0)
    try:
        fm, oc = staged_inputs(e, n, m, B, kw)
        fb, ob = torch.from_numpy(fm.view(np.int32)).cuda(), torch.from_numpy(oc).cuda()
        given = L.make_params(n, m, seed=kw["seed"], first_trial=first)
        for tag, p, ins in (("drawn", L.make_params(n, m, **kw), {}),
                            ("staged", given, dict(d_faulty=fb.data_ptr(), d_order=ob.data_ptr()))):
            entries = [lambda b, e_, v: e.split_votes_device(p, B, level, b, e_, v, stream=s, **ins)]
            if level == 1:
                entries.append(lambda b, e_, v: e.subtree_votes_device(p, B, b, e_, v, stream=s, **ins))
            for i, votes_of in enumerate(entries):
                two = torch.zeros((2 * per, W), dtype=torch.int64, device="cuda")
                votes_of(ub, ub + 2, two.data_ptr())
                full = torch.zeros((units * per, W), dtype=torch.int64, device="cuda")
                votes_of(0, units, full.data_ptr())
                torch.cuda.synchronize()
                assert np.array_equal(two.cpu().numpy().view(np.uint64),
                                      oracle_c.pack_votes(v_or, ub, ub + 2)), (tag, i, "two units")
                assert np.array_equal(full.cpu().numpy().view(np.uint64), oracle_c.pack_votes(v_or)), (tag, i)
                dec = torch.empty(B, dtype=torch.int64, device="cuda")
                out = torch.empty(B, dtype=torch.uint8, device="cuda")
                cnt = torch.zeros(16, dtype=torch.int64, device="cuda")
                outs = dict(d_decisions=dec.data_ptr(), d_outcome=out.data_ptr(), stream=s)
                if i == 1:
                    e.root_from_votes_device(p, B, full.data_ptr(), cnt.data_ptr(), **outs, **ins)
                else:
                    e.root_from_split_votes_device(p, B, level, full.data_ptr(), cnt.data_ptr(), **outs, **ins)
                torch.cuda.synchronize()
                same(dec.cpu().numpy().view(np.uint64), od, f"decisions {tag} {i}")
                same(out.cpu().numpy(), oo, f"outcome {tag} {i}")
                assert cnt.cpu().tolist()[:12] == list(ocnt.values()), (tag, i)
    finally:
        e.close()


# --- ba_gen_inputs_device alone -------------------------------------------------------------
@pytest.mark.parametrize("start", ["T32", "W32", "HI", "TOP"])
@pytest.mark.parametrize("n", [1, 4, 10, 16, 32])
def test_gen_inputs_device(engine, n, start):
    import torch
    from ba_amd import lib as L
    B = 256
    first = {"T32": T32(2), "W32": W32(2), "HI": HI, "TOP": TOP(B)}[start]
    lib = oracle_c.load()
    fb = torch.empty(B, dtype=torch.int32, device="cuda")
    ob = torch.empty(B, dtype=torch.uint8, device="cuda")
    a, b = ctypes.c_uint32(), ctypes.c_uint8()
    for mode, f in ((L.FAULTY_RANDOM, n), (L.FAULTY_RANDOM, (n + 2) // 3), (L.FAULTY_EXACT, n // 2),
                    (L.FAULTY_EXACT, n)):
        seed = 0x5157ED0123456789 + f
        p = L.make_params(n, 1, seed=seed, faulty_mode=mode, f=f, order_mode=L.ORDER_RANDOM,
                          first_trial=first)
        engine.gen_inputs_device(p, B, d_faulty=fb.data_ptr(), d_order=ob.data_ptr(),
                                 stream=torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        fm, oc = fb.cpu().numpy().view(np.uint32), ob.cpu().numpy()
        for i in range(B):
            lib.ba_oracle_gen(n, seed, mode, f, L.ORDER_RANDOM, 1, first + i, ctypes.byref(a), ctypes.byref(b))
            assert (int(fm[i]), int(oc[i])) == (a.value, b.value), (n, mode, f, start, i)
        if mode == L.FAULTY_EXACT:
            assert all(bin(int(x)).count("1") == f for x in fm)


# --- SM(m): k_sm ---------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def sm_case(n, m, first, B):
    """(seed, model results) of an SM case.  SM(m) outputs follow few of the coins, so
    at n <= 16 the seed is the first under which the model's results change when
    every trial word keeps its inputs but loses its upper half (the upper word of
    the coins' counter cleared); (32, 8) keeps one seed (see test_sm)."""
    from ba_amd import lib as L
    for seed in range(0x5157ED, 0x5157ED + 64):
        kw = dict(seed=seed, faulty_mode=L.FAULTY_RANDOM, f=n, order_mode=L.ORDER_RANDOM)
        ref = S.run(n, m, first_trial=first, batch=B, **kw)
        if n > 16 or (first + B - 1) >> 38 == 0:  # (T32: no trial word has an upper half)
            break
        low = []
        for i0 in range(0, B, 64):
            ins = [O.gen(n, seed, O.FAULTY_RANDOM, n, O.ORDER_RANDOM, 1, first + i) for i in range(i0, min(B, i0 + 64))]
            r = S.run(n, m, seed=seed, faulty=[a for a, _ in ins], order=[b for _, b in ins], batch=len(ins),
                      first_trial=(((first + i0) >> 6) & 0xFFFFFFFF) << 6)
            low += r[0]
        if low != ref[0]:
            break
    else:
        raise AssertionError("no seed found")
    dec, out, vs, cnt = ref
    return seed, (np.array(dec, np.uint64), np.array(out, np.uint8), np.array(vs, np.uint64), cnt)


@pytest.mark.parametrize("start", ["W32", "T32", "HI", "TOP"])
@pytest.mark.parametrize("n,m", [(4, 1), (10, 3), (16, 1), (32, 8)])
def test_sm(n, m, start):
    """k_sm against the chain-form model, drawn and staged inputs.  (32, 8) takes the
    kernel's four-pass coin groups, but its outputs hardly depend on the coins (31
    lieutenants hear both values from a faulty commander and relay them: every V
    saturates, under any inputs, since the coins are fair): what it checks above 2^32
    is the input stream.  (16, 1) takes the same four-pass group (210 pairs) with one
    relay round, which leaves V sets that follow the coins; it, (4, 1) and (10, 3)
    run under a seed whose results hang on the coins' upper counter word."""
    from ba_amd import lib as L
    B = 256 if start == "TOP" else 229
    first = {"W32": W32(2), "T32": T32(2), "HI": HI, "TOP": TOP(256)}[start]
    seed, ref = sm_case(n, m, first, B)
    kw = dict(seed=seed, faulty_mode=L.FAULTY_RANDOM, f=n, order_mode=L.ORDER_RANDOM, first_trial=first)
    assert O.FAULTY_RANDOM == L.FAULTY_RANDOM and O.ORDER_RANDOM == L.ORDER_RANDOM
    e = L.Engine(0)
    try:
        e.profile(True)
        check_sm(e.run_sm(n, m, B, want_vsets=True, **kw), ref, f"drawn n={n} m={m} {start}")
        fm, oc = staged_inputs(e, n, m, B, kw)
        check_sm(e.run_sm(n, m, B, seed=kw["seed"], first_trial=first, faulty=fm, order=oc, want_vsets=True),
                 ref, f"staged n={n} m={m} {start}")
        prof = e.profile_read()
    finally:
        e.close()
    assert prof["k_sm"][0] == 2, prof


# --- sharding and trial-DP across the boundary ----------------------------------------------
def test_sharding_across_2_38(engine):
    """One call of 20 words from W32(10) equals two calls of 10: the second starts
    exactly at trial 2^38."""
    kw = kw_for(10, W32(10))
    full = engine.run(10, 3, 64 * 20, **kw)
    parts = [engine.run(10, 3, 64 * 10, **dict(kw, first_trial=W32(10) + 64 * 10 * i)) for i in range(2)]
    assert kw["first_trial"] + 64 * 10 == 2**38
    same(np.concatenate([p.decisions for p in parts]), full.decisions, "decisions")
    same(np.concatenate([p.outcome for p in parts]), full.outcome, "outcome")
    assert {k: sum(p.counters[k] for p in parts) for k in full.counters} == full.counters
    od, oo, ocnt = oracle(10, 3, 64 * 20, W32(10))
    same(full.decisions, od, "decisions vs oracle")
    same(full.outcome, oo, "outcome vs oracle")
    assert {k: full.counters[k] for k in ocnt} == ocnt


def test_run_trials_multi_world1(engine):
    """ba_run_trials_multi over a one-rank communicator (first_trial + share first)."""
    import torch
    from ba_amd import lib as L
    n, m, B = 10, 3, 64 * 6 + 9
    dec = torch.empty(B, dtype=torch.int64, device="cuda")
    out = torch.empty(B, dtype=torch.uint8, device="cuda")
    comm = L.Comm(engine, 1, 0, L.comm_unique_id())
    try:
        for first in (W32(2), T32(2), HI):
            cnt, sf, sc = comm.run_trials(L.make_params(n, m, **kw_for(n, first)), B, dec.data_ptr(),
                                          out.data_ptr())
            torch.cuda.synchronize()
            assert (sf, sc) == (0, B)
            od, oo, ocnt = oracle(n, m, B, first)
            same(dec.cpu().numpy().view(np.uint64), od, f"decisions first_trial={first}")
            same(out.cpu().numpy(), oo, f"outcome first_trial={first}")
            assert {k: cnt[k] for k in ocnt} == ocnt, first
    finally:
        comm.close()


def test_run_trials_multi_three_ranks_across_2_38(tmp_path_factory):
    """Three ranks over six words from W32(2) (tests/multirank.py, the RCCL stand-in):
    rank 1's share starts exactly at trial 2^38, rank 2's past it.  The ranks' run is
    the one tests/test_multirank_gpu.py makes (shared, not repeated)."""
    import multirank as MR
    from test_multirank_gpu import oracle as mr_oracle, ranks
    case = (10, 3, 64 * 6, 5, W32(2))
    k = MR.DP_CASES.index(case)
    n, m, total, f, first = case
    od, oo, ocnt = mr_oracle(n, m, total, f, first)
    res = ranks(3, tmp_path_factory)
    assert sorted(first + r["dp"][k]["first"] for r in res) == [W32(2), 2**38, 2**38 + 128]
    for r in res:
        g = r["dp"][k]
        assert g["case"] == list(case) and g["count"] == 128
        s = g["first"]
        same(np.array(g["dec"], np.uint64), od[s:s + 128], f"decisions rank {r['rank']}")
        same(np.array(g["out"], np.uint8), oo[s:s + 128], f"outcome rank {r['rank']}")
        assert {c: g["counters"][c] for c in ocnt} == ocnt, r["rank"]
