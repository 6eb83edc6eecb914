"""GPU parity of k_om3wt's byte-sliced input staging and result pick-out
(n = 10, m = 3; csrc/ba_bitslice.hpp, stage_words_sliced and
wave_epilogue_sliced in csrc/ba_wave.hpp).

In k_om3wt lane (w, k) loads the 8 trials of byte k of word w with wide loads,
transposes them into the input planes in registers, and at the end transposes
its 8 trials' root and outcome bytes into decision words and outcome bytes and
stores them itself.  k_om3w (BA_OM3W_TABLE=0) keeps the ballot staging and the
per-bit pick-out and is the A/B reference on arbitrary inputs; oracle_c.run is
the reference on the protocol's own inputs.

  * oracle parity, staged inputs and in-kernel draws, at batches that reach
    every tail case -- a lane partly valid (1, 7, 9, 63, 65, 511, 513), a lane
    empty, a word partly valid, a task partly valid, one wave walking several
    tasks (5 * 512 + 37 under BA_WAVE_MAX_BLOCKS=1) -- with first_trial 64 * 9
    and 64 * (2^32 + 16);
  * old path versus new on arbitrary given inputs: full 32-bit faulty masks
    (only the low n bits count) and order bytes over all 256 values (1 = attack,
    2 = no order, anything else retreat), identical decisions, outcomes and
    counters, and profile_read names the kernel that ran;
  * the same with every buffer off its natural wide alignment: d_faulty by 1-3
    elements, d_order by 1-7 bytes, d_decisions by one element, d_outcome by 1-7
    bytes (only the C ABI's element alignment may be assumed);
  * no stray stores: sentinels behind the batch and in front of an offset
    pointer survive; a null d_outcome or d_decisions leaves the other output
    equal to the oracle's.
"""
import numpy as np
import pytest

import oracle_c
from test_gpu import same
from test_gpu_om3w_table import FT_HI1, FT_LOW, check_case, kw_for

pytestmark = pytest.mark.gpu

N, M, W = 10, 3, 8
TASK = 64 * W
BATCHES = [(1, None), (7, None), (8, None), (9, None), (63, None), (64, None), (65, None),
           (TASK - 1, None), (TASK, None), (TASK + 1, None), (5 * TASK + 37, "1")]
DEC_SENTINEL, OUT_SENTINEL = -0x0123456789ABCDEF, 0xA5
PAD, PREFIX = 128, 64


@pytest.mark.parametrize("first_trial", [FT_LOW, FT_HI1], ids=["ft_low", "ft_hi1"])
@pytest.mark.parametrize("B,cap", BATCHES)
def test_tail_batches_vs_oracle(monkeypatch, B, cap, first_trial):
    monkeypatch.delenv("BA_OM3W_TABLE", raising=False)
    if cap:
        monkeypatch.setenv("BA_WAVE_MAX_BLOCKS", cap)
    else:
        monkeypatch.delenv("BA_WAVE_MAX_BLOCKS", raising=False)
    check_case(N, B, kw_for(first_trial, seed=0x10A + B), "k_om3wt",
               f"B={B} cap={cap} first_trial={first_trial}")


class Buffers:
    """Device buffers of one run: inputs at element offsets (fo, oo), outputs at
    (do, uo) behind a 64-element sentinel prefix and with 128 sentinel elements
    behind the batch."""

    def __init__(self, faulty, order, fo=0, oo=0, do=0, uo=0):
        import torch
        B = len(faulty)
        self.B, self.do, self.uo = B, PREFIX + do, PREFIX + uo
        fb = np.zeros(B + fo, np.uint32)
        fb[fo:] = faulty
        ob = np.zeros(B + oo, np.uint8)
        ob[oo:] = order
        self.fb = torch.from_numpy(fb.view(np.int32)).cuda()
        self.ob = torch.from_numpy(ob).cuda()
        self.dec = torch.full((self.do + B + PAD,), DEC_SENTINEL, dtype=torch.int64, device="cuda")
        self.out = torch.full((self.uo + B + PAD,), OUT_SENTINEL, dtype=torch.uint8, device="cuda")
        self.cnt = torch.zeros(16, dtype=torch.int64, device="cuda")
        self.p_f = self.fb.data_ptr() + 4 * fo
        self.p_o = self.ob.data_ptr() + oo
        self.p_dec = self.dec.data_ptr() + 8 * self.do
        self.p_out = self.out.data_ptr() + self.uo

    def run(self, engine, seed, first_trial, decisions=True, outcome=True):
        import torch
        from ba_amd import lib as L
        p = L.make_params(N, M, seed=seed, first_trial=first_trial)
        engine.run_device(p, self.B, d_faulty=self.p_f, d_order=self.p_o,
                          d_decisions=self.p_dec if decisions else 0,
                          d_outcome=self.p_out if outcome else 0, d_counters=self.cnt.data_ptr(),
                          stream=torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        return self

    def results(self):
        dec, out = self.dec.cpu().numpy(), self.out.cpu().numpy()
        return (dec[self.do:self.do + self.B].view(np.uint64), out[self.uo:self.uo + self.B],
                self.cnt.cpu().tolist()[:12])

    def check_sentinels(self, tag, decisions=True, outcome=True):
        dec, out = self.dec.cpu().numpy(), self.out.cpu().numpy()
        lo_d = self.do if decisions else len(dec)
        lo_o = self.uo if outcome else len(out)
        assert (dec[:lo_d] == DEC_SENTINEL).all(), f"{tag}: store in front of d_decisions"
        assert (out[:lo_o] == OUT_SENTINEL).all(), f"{tag}: store in front of d_outcome"
        assert (dec[self.do + self.B:] == DEC_SENTINEL).all(), f"{tag}: decisions stored beyond batch"
        assert (out[self.uo + self.B:] == OUT_SENTINEL).all(), f"{tag}: outcomes stored beyond batch"


def arbitrary_inputs(B, seed):
    rng = np.random.default_rng(seed)
    fm = rng.integers(0, 1 << 32, B, dtype=np.uint64).astype(np.uint32)
    oc = rng.integers(0, 256, B, dtype=np.uint64).astype(np.uint8)
    oc[: 3 * 256] = np.tile(np.arange(256, dtype=np.uint8), 3)[: min(B, 3 * 256)]  # every byte value
    return fm, oc


def ran(engine):
    return sorted(k for k in engine.profile_read() if k.startswith("k_om3w"))


def test_old_path_equals_new_on_arbitrary_inputs_at_any_alignment(monkeypatch):
    from ba_amd import lib as L
    monkeypatch.delenv("BA_WAVE_MAX_BLOCKS", raising=False)
    B, seed, ft = 2 * TASK + 11, 0x5EED10, FT_LOW
    fm, oc = arbitrary_inputs(B, 10)
    e = L.Engine(0)
    try:
        monkeypatch.setenv("BA_OM3W_TABLE", "0")
        e.profile(True)
        old = Buffers(fm, oc).run(e, seed, ft)
        assert ran(e) == ["k_om3w"], e.profile_read()
        old.check_sentinels("old path")
        want = old.results()
        assert want[2][0] == B  # trials
        # the masks' high bits and the odd order bytes are not what decided it
        od, oo, ocnt = oracle_c.run(N, M, B, seed=seed, faulty=fm & ((1 << N) - 1),
                                    order=np.where(oc <= 2, oc, 0).astype(np.uint8), first_trial=ft)
        same(want[0], od, "old path vs oracle on the canonical inputs: decisions")
        same(want[1], oo, "old path vs oracle on the canonical inputs: outcome")
        assert want[2] == list(ocnt.values())
        monkeypatch.delenv("BA_OM3W_TABLE")
        # aligned, then every buffer off its wide alignment
        offsets = [(0, 0, 0, 0)] + [((k - 1) % 3 + 1, k, 1, k) for k in range(1, 8)]
        for fo, oo_, do, uo in offsets:
            tag = f"offsets faulty={fo} order={oo_} decisions={do} outcome={uo}"
            e.profile(True)
            new = Buffers(fm, oc, fo, oo_, do, uo).run(e, seed, ft)
            assert ran(e) == ["k_om3wt"], e.profile_read()
            dec, out, cnt = new.results()
            same(dec, want[0], "decisions, " + tag)
            same(out, want[1], "outcome, " + tag)
            assert cnt == want[2], tag
            new.check_sentinels(tag)
    finally:
        e.close()


@pytest.mark.parametrize("B", [1, 65, TASK + 1])
def test_no_stray_stores_and_null_outputs(monkeypatch, B):
    from ba_amd import lib as L
    monkeypatch.delenv("BA_OM3W_TABLE", raising=False)
    monkeypatch.delenv("BA_WAVE_MAX_BLOCKS", raising=False)
    rng = np.random.default_rng(B)
    fm = (rng.integers(0, 1 << N, B, dtype=np.uint64) & rng.integers(0, 1 << N, B, dtype=np.uint64)).astype(np.uint32)
    oc = rng.choice([0, 1, 2], B).astype(np.uint8)
    seed, ft = 0xB0B + B, FT_LOW
    od, oo, ocnt = oracle_c.run(N, M, B, seed=seed, faulty=fm, order=oc, first_trial=ft)
    e = L.Engine(0)
    try:
        e.profile(True)
        for do, uo in ((0, 0), (1, 3)):
            tag = f"B={B} offsets decisions={do} outcome={uo}"
            both = Buffers(fm, oc, 0, 0, do, uo).run(e, seed, ft)
            dec, out, cnt = both.results()
            same(dec, od, "decisions, " + tag)
            same(out, oo, "outcome, " + tag)
            assert cnt == list(ocnt.values()), tag
            both.check_sentinels(tag)
            no_out = Buffers(fm, oc, 0, 0, do, uo).run(e, seed, ft, outcome=False)
            same(no_out.results()[0], od, "decisions with a null d_outcome, " + tag)
            assert no_out.results()[2] == list(ocnt.values()), tag
            no_out.check_sentinels(tag + " (null d_outcome)", outcome=False)
            no_dec = Buffers(fm, oc, 0, 0, do, uo).run(e, seed, ft, decisions=False)
            same(no_dec.results()[1], oo, "outcome with a null d_decisions, " + tag)
            assert no_dec.results()[2] == list(ocnt.values()), tag
            no_dec.check_sentinels(tag + " (null d_decisions)", decisions=False)
        assert ran(e) == ["k_om3wt"], e.profile_read()
    finally:
        e.close()
