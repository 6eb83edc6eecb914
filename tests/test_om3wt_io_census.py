"""Static census of the input staging and result pick-out of k_om3wt<10, staged>.

Both are 64 x 8-bit matrix transposes.  k_om3w does them a bit at a time: 13
ballots and 26 v_writelane_b32 per word to stage the inputs (~460 VALU per
task), one bfe + shift-or per output bit to pick the results out (~312).
k_om3wt does them in the layout lane = (word, byte) with 8x8 bit transposes in
registers (csrc/ba_bitslice.hpp; stage_words_sliced and wave_epilogue_sliced in
csrc/ba_wave.hpp): three wide loads and five wide stores per lane, no
writelane, no LDS round trip of the outcome planes.

The kernel's straight-line blocks are classified by what only they contain:
  staging   the blocks from the first global load up to and including the block
            with the byte stores of the planes into LDS (ds_write_b8), before
            the round block; the guarded tail path is the loop among them that
            loads a dword and a byte per trip, the full-lane path the wide loads
  pick-out  the full-lane path behind the rounds: the epilogue block, the wide
            stores, and the blocks with the run counters' popcounts and the
            packed fold; epilogue_core's own count (with the fold) is taken
            from k_om3w<10, staged>, where epilogue phase 1 and the fold are
            blocks of their own on either side of the pick-out loop.
Budgets are this build's counts; the issue's bounds (two or three 21-instruction
transposes plus packing, with headroom: 150 each) are asserted on top.
"""
import collections

import codeobj
from test_om3w_census import BENCH_KERNEL as OM3W_KERNEL, straight_line_blocks
from test_om3wt_census import KERNEL, KERNEL_VALU_BUDGET as PARENT_KERNEL_VALU

STAGING_VALU_BUDGET = 150
PICKOUT_VALU_BUDGET = 150
KERNEL_VALU = 1941            # this build, static; the parent build had 2,21x
MAX_STAGING_LOADS = 4         # full-lane path: 2 x dwordx4 (masks) + 1 x dwordx2 (order bytes)
MAX_PICKOUT_STORES = 6        # full-lane path: 4 x dwordx4 (decisions) + 1 x dwordx2 (outcomes)


def valu(block):
    return sum(1 for i in block if i.startswith("v_"))


def count(block, prefix):
    return sum(1 for i in block if i.startswith(prefix))


def round_index(blocks):
    (r,) = [k for k, b in enumerate(blocks) if count(b, "v_mad_u64_u32") >= 300]
    return r


def core_blocks(blocks, after):
    """The blocks behind the round block that hold the run counters' popcounts
    (v_bcnt_u32_b32: the end of epilogue_core) and the packed fold's DPP adds."""
    return [k for k in range(after, len(blocks))
            if count(blocks[k], "v_bcnt_u32_b32") or any("_dpp" in i for i in blocks[k])]


def census(lib_path=codeobj.LIB):
    def kernel(prefix):
        found = []
        for co in codeobj.code_objects(lib_path):
            for name, ins in codeobj.functions(codeobj.disassemble(co)).items():
                if name.startswith(prefix):
                    found.append(ins)
        (ins,) = found
        return ins

    ins = kernel(KERNEL)
    blocks = straight_line_blocks(ins)
    r = round_index(blocks)
    before = blocks[:r]
    # ---- staging ---------------------------------------------------------------
    first = min(k for k, b in enumerate(before) if count(b, "global_load"))
    last = max(k for k, b in enumerate(before) if count(b, "ds_write_b8"))
    staging = before[first:last + 1]
    tail = [b for b in staging if count(b, "global_load_ubyte")]
    full = [b for b in staging if count(b, "global_load") and b not in tail]
    # the tail loop is skipped by the full lanes: its trips and the block that
    # zeroes its registers do not run for them
    tail_ix = [k for k, b in enumerate(staging) if b in tail]
    skipped = staging[max(0, tail_ix[0] - 1):tail_ix[-1] + 2] if tail_ix else []
    c = {
        "writelanes_before_rounds": sum(count(b, "v_writelane_b32") for b in before[1:]),
        "writelanes_entry_block": count(before[0], "v_writelane_b32"),
        "staging_valu_full_lane": sum(valu(b) for b in staging if b not in skipped),
        "staging_valu_static": sum(valu(b) for b in staging),
        "staging_loads_full_lane": sum(count(b, "global_load") for b in full),
        "staging_loads_tail": sum(count(b, "global_load") for b in tail),
        "staging_wide_loads": sum(count(b, "global_load_dwordx") for b in full),
    }
    # ---- pick-out --------------------------------------------------------------
    # the full-lane path: the epilogue block (the large block in front of the
    # stores), the block with the dwordx4 decision stores and the store blocks that
    # follow it back to back (the outcomes), then -- behind the guarded per-trial
    # loop, which the full lanes skip -- the popcounts and the fold, which the
    # compiler sinks below the stores
    stores = [k for k in range(r + 1, len(blocks)) if count(blocks[k], "global_store")]
    wide = [min(k for k in stores if count(blocks[k], "global_store_dwordx4"))]
    while wide[-1] + 1 in stores:
        wide.append(wide[-1] + 1)
    e = max(k for k in range(r + 1, wide[0]) if valu(blocks[k]) >= 100)
    core = core_blocks(blocks, r + 1)
    full_path = blocks[e:wide[-1] + 1] + [blocks[k] for k in core if k > wide[-1]]
    assert not any(count(b, "global_store_byte") for b in full_path)
    # k_om3w: epilogue phase 1 and the fold, without its pick-out loop between them
    om3w = straight_line_blocks(kernel(OM3W_KERNEL))
    core_valu = sum(valu(om3w[k]) for k in core_blocks(om3w, round_index(om3w) + 1))
    c.update({
        "epilogue_path_valu_full_lane": sum(valu(b) for b in full_path),
        "om3w_epilogue_core_and_fold_valu": core_valu,
        "pickout_valu_full_lane": sum(valu(b) for b in full_path) - core_valu,
        "pickout_stores_full_lane": sum(count(b, "global_store") for b in full_path),
        "pickout_stores_tail": sum(count(blocks[k], "global_store") for k in stores
                                   if k > wide[-1]),
        "kernel_valu": valu(ins),
        "kernel_ops_io": dict(collections.Counter(
            i.split()[0] for i in ins if i.startswith(("global_load", "global_store")))),
    })
    return c


def test_staging_and_pickout_census():
    c = census()
    print(c)
    # no writelane in front of the rounds but the kernel entry's SGPR spills (kernel
    # arguments parked in VGPR lanes before the task loop, as in k_om3w)
    assert c["writelanes_before_rounds"] == 0, c
    (res,) = [v for k, v in codeobj.kernel_resources().items() if k.startswith(KERNEL)]
    assert c["writelanes_entry_block"] <= res["sgpr_spill"], (c, res)
    assert c["staging_loads_full_lane"] <= MAX_STAGING_LOADS, c
    assert c["staging_wide_loads"] == c["staging_loads_full_lane"], c
    assert c["staging_valu_full_lane"] <= STAGING_VALU_BUDGET, c
    assert c["pickout_stores_full_lane"] <= MAX_PICKOUT_STORES, c
    assert c["pickout_valu_full_lane"] <= PICKOUT_VALU_BUDGET, c
    assert KERNEL_VALU < PARENT_KERNEL_VALU - 250
    assert c["kernel_valu"] <= KERNEL_VALU, c
