"""Static instruction census of k_om3wt<10, staged>, the bench kernel with the
wave-shared Philox pair table (csrc/ba_wave.hpp, Om3PairTable).

Against k_om3w's round (tests/test_om3w_census.py: 1,205 VALU, 450
v_mad_u64_u32 = 25 calls x 18), the 21 leaf calls of a round take the pair-only
half of their rounds 0-1 from the table: per call two multiplies, two xor3 and
the counter add go, two 2-input xors come (42 v_xor_b32 per round), and the
table build adds three passes per round for the whole wave.  Multiplies: the
issue's count is 450 - 2 x 21 served calls + the build's multiplies.  A build
pass is two products (M0 pair, M1 z1), six per round as written; the compiler
keeps M0 pair as a running 64-bit sum across passes and rounds (the pairs step
by constants), so fewer remain: 413 in this build (400 in the rounds 2-9
statements of the 25 calls, 13 in the diagonal group's rounds 0-1 and the
build), held exactly, and never above 450 - 42 + 6.

The round stays one straight-line block, with no spill at <= 168 VGPRs (three
waves per SIMD), for the staged and the in-kernel-input variant.  Budgets are
this build's counts; the round budget must stay below 1,205 - 40.
"""
import collections

import codeobj
from test_om3w_census import PROTOCOL_OPS, ROUND_VALU_BUDGET as OM3W_ROUND_VALU, straight_line_blocks

KERNEL = "_ZN2ba7k_om3wtILi10ELb1EE"      # staged: the bench's launch
KERNEL_DRAWN = "_ZN2ba7k_om3wtILi10ELb0EE"
LEAF_CALLS = 21                            # served from the table, per round
BUILD_MULTIPLIES_WRITTEN = 6               # 3 passes x (M0 pair, M1 z1)
ROUND_MAD = 413
ROUND_VALU_BUDGET = 1152
ROUND_OTHER_BUDGET = 124                   # of them 42 v_xor_b32: the calls' own two xors
KERNEL_VALU_BUDGET = 2220


def kernels(prefix):
    found = []
    for co in codeobj.code_objects():
        for name, ins in codeobj.functions(codeobj.disassemble(co)).items():
            if name.startswith(prefix):
                found.append(ins)
    return found


def test_round_block_and_kernel_valu_budgets():
    found = kernels(KERNEL)
    assert len(found) == 1, len(found)
    ins = found[0]
    rounds = [b for b in straight_line_blocks(ins)
              if sum(1 for i in b if i.startswith("v_mad_u64_u32")) >= 300]
    assert len(rounds) == 1, [len(b) for b in rounds]
    ops = collections.Counter(i.split()[0] for i in rounds[0] if i.startswith("v_"))
    other = {k: n for k, n in ops.items() if k not in PROTOCOL_OPS}
    c = {"round_valu": sum(ops.values()), "round_other": sum(other.values()),
         "kernel_valu": sum(1 for i in ins if i.startswith("v_")), "round_ops": dict(ops)}
    print(c)
    assert ROUND_VALU_BUDGET < OM3W_ROUND_VALU - 40
    assert ops["v_mad_u64_u32"] == ROUND_MAD, c
    assert ops["v_mad_u64_u32"] <= 450 - 2 * LEAF_CALLS + BUILD_MULTIPLIES_WRITTEN, c
    assert ops["v_xor_b32_e32"] == 2 * LEAF_CALLS, c
    assert c["round_valu"] <= ROUND_VALU_BUDGET, c
    assert c["round_other"] <= ROUND_OTHER_BUDGET, c
    assert c["kernel_valu"] <= KERNEL_VALU_BUDGET, c
    # the whole round's table traffic: 3 build passes, 21 entries read back
    lds = collections.Counter(i.split()[0] for i in rounds[0] if i.startswith("ds_"))
    assert not any(i.startswith("scratch_") for i in ins), "spill code in the kernel"
    assert sum(lds.values()) <= 50, lds


def test_no_spills_and_three_waves_per_simd():
    res = codeobj.kernel_resources()
    for prefix in (KERNEL, KERNEL_DRAWN):
        (r,) = [v for k, v in res.items() if k.startswith(prefix)]
        assert r["vgpr_spill"] == 0 and r["vgpr"] <= 168, (prefix, r)
