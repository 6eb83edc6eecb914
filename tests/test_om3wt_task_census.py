"""Static census of what a task of k_om3wt<10, staged> executes around the nine
passes of its round block (tests/test_om3wt_census.py pins that block itself).

The kernel is bound by VALU issue, so the per-task code outside the rounds is
counted the same way, from the disassembly with its branch targets resolved:

  round loop   the blocks from the target of the back-edges that span the round
               block (the block with >= 300 v_mad_u64_u32) to the last of those
               back-edges; "per round" is every block of the loop but the round
               block: loop control, priority, the L0 load, the R1 majority of
               om3_round, the R1T store (static: every block counted once)
  setup        the blocks between the level-0 block (the one with the 20
               multiplies of level 0's Philox calls) and the loop: the lane
               tables, the E row, the pair table's lane fields, the addresses
               the rounds use
  roots        from the loop's exit to the last LDS store in front of the
               epilogue's global stores: the root majorities

In the parent build the roots were a loop of two exec-masked trips of a 64-bit
carry-save count (1 + 2 x 48 VALU per task) and the lane tables a ladder of
compares, selects and ors.  Now the roots are three straight-line trips of a
32-bit count over half-columns (Om3RootHalves, csrc/ba_om3_task.hpp), the
tables closed forms (om3_lane_tables), and no `act` select remains outside
om3_round.  Budgets are this build's counts; each must stay below the parent's.
"""
import re

import codeobj
from test_om3wt_census import KERNEL

PARENT_SETUP_VALU = 109        # 7 + 13 (E row under `act`) + 89
PARENT_PER_ROUND_VALU = 37     # static, the loop's blocks without the round block (36 on
                               # the path with lanes active; 1 in the `!act` block)
PARENT_ROOTS_VALU = 97         # 1 + 2 trips x 48
SETUP_VALU_BUDGET = 69
PER_ROUND_VALU_BUDGET = 34
ROOTS_VALU_BUDGET = 51
BRANCHES = ("s_branch", "s_setpc_b64", "s_endpgm")


def kernel_blocks(lib_path=codeobj.LIB):
    """[(start address, [(address, instruction, branch target or None), ...]), ...]:
    the kernel's straight-line blocks in layout order."""
    found = []
    for co in codeobj.code_objects(lib_path):
        ins, on, base = [], False, 0
        for line in codeobj.disassemble(co).splitlines():
            m = re.match(r"^([0-9a-f]+) <(.+)>:$", line)
            if m:
                on, base = m.group(2).startswith(KERNEL), int(m.group(1), 16)
                if on:
                    found.append(ins)
                continue
            if not (on and line.startswith("\t")):
                continue
            text, _, note = line.partition("//")
            a = re.match(r"\s*([0-9A-Fa-f]+):", note)
            if not text.strip() or not a:
                continue
            t = re.search(r"<[^>]*\+0x([0-9a-f]+)>\s*$", note)
            ins.append((int(a.group(1), 16), text.strip(), base + int(t.group(1), 16) if t else None))
    (ins,) = [f for f in found if f]
    blocks, cur = [], []
    for i in ins:
        cur.append(i)
        op = i[1].split()[0]
        if op.startswith("s_cbranch") or op in BRANCHES:
            blocks.append((cur[0][0], cur))
            cur = []
    if cur:
        blocks.append((cur[0][0], cur))
    return blocks


def valu(instrs):
    return sum(1 for _, i, _ in instrs if i.startswith("v_"))


def count(instrs, prefix):
    return sum(1 for _, i, _ in instrs if i.startswith(prefix))


def back_edge(block):
    """The target of the block's closing branch if it jumps backwards."""
    a, _, target = block[1][-1]
    return target if target is not None and target <= a else None


def census(lib_path=codeobj.LIB):
    blocks = kernel_blocks(lib_path)
    (r,) = [k for k, (_, b) in enumerate(blocks) if count(b, "v_mad_u64_u32") >= 300]
    level0 = max(k for k in range(r) if count(blocks[k][1], "v_mad_u64_u32") >= 20)
    # the round loop: back-edges from at or behind the round block to at or in front of
    # it, but behind level 0 (the task loop's own back-edges reach in front of that)
    spans = [(k, back_edge(b)) for k, b in enumerate(blocks)
             if k >= r and back_edge(b) is not None
             and blocks[level0][0] < back_edge(b) <= blocks[r][0]]
    assert spans, "no back-edge spans the round block"
    head_addr = min(t for _, t in spans)
    head = max(k for k, (a, _) in enumerate(blocks) if a <= head_addr)
    last = max(k for k, _ in spans)
    assert head <= r <= last
    per_round = [k for k in range(head, last + 1) if k != r]
    # setup: behind the level-0 block, in front of the loop
    assert level0 < head
    setup = list(range(level0 + 1, head))
    # roots: from the loop's exit to the last LDS store in front of the global stores
    store = min(k for k in range(last + 1, len(blocks)) if count(blocks[k][1], "global_store"))
    tail = [i for k in range(last + 1, store) for i in blocks[k][1]]
    writes = [n for n, (_, i, _) in enumerate(tail) if i.startswith("ds_write")]
    assert writes, "no root store behind the rounds"
    roots = tail[:writes[-1] + 1]
    epilogue = min(k for k in range(last + 1, store + 1) if valu(blocks[k][1]) >= 100)
    loops = [k for k in range(last + 1, epilogue + 1) if back_edge(blocks[k]) is not None]
    return {
        "setup_valu": sum(valu(blocks[k][1]) for k in setup),
        "per_round_valu": sum(valu(blocks[k][1]) for k in per_round),
        "roots_valu": valu(roots),
        "roots_lds_reads": count(roots, "ds_read"),
        "roots_quarter_rate_multiplies": count(roots, "v_mul_lo_u32") + count(roots, "v_mul_hi_u32"),
        "back_edges_between_rounds_and_epilogue": len(loops),
        "blocks": {"round": r, "loop": (head, last), "setup": setup, "epilogue": epilogue},
    }


def test_task_census():
    c = census()
    print(c)
    assert SETUP_VALU_BUDGET < PARENT_SETUP_VALU
    assert PER_ROUND_VALU_BUDGET < PARENT_PER_ROUND_VALU
    assert ROOTS_VALU_BUDGET < PARENT_ROOTS_VALU
    assert c["setup_valu"] <= SETUP_VALU_BUDGET, c
    assert c["per_round_valu"] <= PER_ROUND_VALU_BUDGET, c
    assert c["roots_valu"] <= ROOTS_VALU_BUDGET, c
    assert c["roots_quarter_rate_multiplies"] == 0, c
    # the roots are straight-line code: no loop between the round loop and the epilogue
    assert c["back_edges_between_rounds_and_epilogue"] == 0, c
