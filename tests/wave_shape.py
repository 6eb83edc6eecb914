"""The launch shape of the WAVE engines, mirrored from launch_wave (csrc/ba_wave.hpp):
how many tasks a batch makes, how many blocks take them, and whether some wave
therefore walks the kernel's task loop more than once.  The tests that claim the
loop assert it from here, so a later change of their batch cannot silently leave
the loop again.

    words  = ceil(B / 64)
    tasks  = ceil(words / W)            one wave resolves a task of W words
    blocks = min(ceil(tasks / 4), cap)  4 waves per block; cap = BPC * cu_count, or
                                        BA_WAVE_MAX_BLOCKS when that is in [1, cap)
    persistent = tasks > 4 * blocks
"""
from collections import namedtuple

WAVES_PER_BLOCK = 4   # kWaveThreads / 64
CU_COUNT = 256        # the ba_ctx default (MI355X)
OM4W_BPC = 3          # BA_OM4W_BLOCKS_PER_CU: k_om4w's launch cap, blocks per CU
OM3W_BPC = 2          # Om3W<N>::BPC

WaveShape = namedtuple("WaveShape", "words tasks blocks persistent")


def om4w_words(n):
    """Om4W<N>::W: the words of one k_om4w task."""
    return 64 // (n - 3)


def cu_count(engine=0):
    """The compute units launch_wave sizes its default cap with: the device's count, as
    a ctx reads it at ba_ctx_create (`engine`: an L.Engine, or a device index), and the
    ctx default where the device reports none."""
    import torch
    cus = torch.cuda.get_device_properties(getattr(engine, "device", engine)).multi_processor_count
    return cus if cus > 0 else CU_COUNT


def wave_shape(W, B, cap=None, cu_count=CU_COUNT, bpc=OM4W_BPC):
    """(words, tasks, blocks, persistent) of a launch of B trials in tasks of W words;
    cap: the value of BA_WAVE_MAX_BLOCKS (None or "": unset)."""
    words = (B + 63) // 64
    tasks = (words + W - 1) // W
    blocks = (tasks + WAVES_PER_BLOCK - 1) // WAVES_PER_BLOCK
    limit = bpc * cu_count
    if cap not in (None, ""):
        c = int(cap, 0) if isinstance(cap, str) else int(cap)
        if 1 <= c < limit:
            limit = c
    blocks = min(blocks, limit)
    return WaveShape(words, tasks, blocks, tasks > blocks * WAVES_PER_BLOCK)
