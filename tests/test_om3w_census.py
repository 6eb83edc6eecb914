"""Static instruction census of the shipped bench kernel k_om3w<10, 0, staged>.

The kernel is issue-bound: what moves the bench is the
number of VALU instructions per task.  A first-hop round is one straight-line
block holding its 450 v_mad_u64_u32; of its VALU instructions, the multiplies,
the v_bitop3_b32 (Philox xor3 and carry-save) and the v_bfi_b32 (relay selects)
are the protocol's work, and everything else is bookkeeping: register copies,
re-materialised constants, address arithmetic, the pair exchange.  This test
holds the round block's VALU count, its bookkeeping count and the kernel's
whole static VALU count at what the build has now, so a change that brings
copies back shows up without a GPU.

The budgets are this build's counts.  Before the Philox groups alternated
register windows and the counter fold packed two counters per dword, the same
census read 1230 / 104 / 2400.
"""
import collections
import re

import codeobj

BENCH_KERNEL = "_ZN2ba6k_om3wILi10ELi0ELb1EE"
PROTOCOL_OPS = ("v_mad_u64_u32", "v_bitop3_b32", "v_bfi_b32")
ROUND_VALU_BUDGET = 1205      # straight-line round block, every v_* instruction
ROUND_OTHER_BUDGET = 79       # ... of them outside PROTOCOL_OPS
KERNEL_VALU_BUDGET = 2255     # the whole kernel, static
PARENT_ROUND_VALU, PARENT_ROUND_OTHER = 1232, 106


def bench_kernel():
    found = []
    for co in codeobj.code_objects():
        for name, ins in codeobj.functions(codeobj.disassemble(co)).items():
            if name.startswith(BENCH_KERNEL):
                found.append(ins)
    assert len(found) == 1, len(found)
    return found[0]


def straight_line_blocks(ins):
    blocks, cur = [], []
    for i in ins:
        cur.append(i)
        op = i.split()[0]
        if op.startswith("s_cbranch") or op in ("s_branch", "s_endpgm", "s_setpc_b64"):
            blocks.append(cur)
            cur = []
    if cur:
        blocks.append(cur)
    return blocks


def census():
    ins = bench_kernel()
    rounds = [b for b in straight_line_blocks(ins)
              if sum(1 for i in b if i.startswith("v_mad_u64_u32")) >= 400]
    assert len(rounds) == 1, [len(b) for b in rounds]
    ops = collections.Counter(i.split()[0] for i in rounds[0] if i.startswith("v_"))
    other = {k: n for k, n in ops.items() if k not in PROTOCOL_OPS}
    return {"round_valu": sum(ops.values()), "round_other": sum(other.values()),
            "kernel_valu": sum(1 for i in ins if i.startswith("v_")),
            "round_ops": dict(ops), "round_other_ops": other,
            "round_copies": sum(1 for i in rounds[0] if re.fullmatch(r"v_mov_b32_e32 v\d+, v\d+", i))}


def test_round_block_and_kernel_valu_budgets():
    c = census()
    print(c)
    assert ROUND_VALU_BUDGET < PARENT_ROUND_VALU and ROUND_OTHER_BUDGET < PARENT_ROUND_OTHER
    # the protocol's own work per round is fixed by the lie stream and the tree
    assert c["round_ops"]["v_mad_u64_u32"] == 450, c["round_ops"]
    assert c["round_valu"] <= ROUND_VALU_BUDGET, c
    assert c["round_other"] <= ROUND_OTHER_BUDGET, c
    assert c["kernel_valu"] <= KERNEL_VALU_BUDGET, c
