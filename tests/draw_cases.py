"""The draw cases the CPU tests (tests/test_draw.py: the wave emulator) and the GPU tests (tests/test_draw_gpu.py: the device) share,
each against the restatement (tests/draw_check.py) -- test infrastructure only.  A case of the normal rows is (nenv, A, a row stride, an
env_base, a seed); its reference is three calls in a row over the whole batch, computed once and never changed."""
import functools

import numpy as np

import draw_check as dc

F32 = np.float32
NENVS = (1, 63, 64, 65, 130)
WIDTHS = (1, 3, 4, 5, 10, 64)
SENTINEL = F32(-77.5)                     # what a word that nobody may touch holds
CALLS = 3
CUTS = ((0, 17), (17, 47), (64, None))    # the ranges of a batch of 130 envs (64 to the end), issued in any order
PERM_NS = (1, 2, 3, 5, 63, 64, 65, 1000, 4095, 4096, 4097, 98304)
PERM_EMU_MAX = 4097                       # the emulator runs the shuffles up to here
SEED = 0x0123456789ABCDEF


def case(nenv, A):
    """(row stride, env_base, seed) of the case: the stride larger than A -- a multiple of 4 words (the 16-byte stores) where A is --,
    env_base not 0 and once next to the wrap of the counter's first word."""
    stride = A + (4 if A % 4 == 0 else 3)
    env_base = 0xFFFFFFF0 if (nenv, A) == (130, 10) else 1000 * nenv + A
    return stride, env_base, SEED ^ (nenv << 8) ^ A


@functools.lru_cache(maxsize=None)
def reference(nenv, A):
    """The rows after each of CALLS calls over the whole batch and the counts after the last: made once, shared, never changed."""
    stride, env_base, seed = case(nenv, A)
    ref = dc.Draws(nenv, A, seed, env_base, stride, fill=SENTINEL)
    rows = []
    for _ in range(CALLS):
        rows.append(ref.draw().copy())
        rows[-1].setflags(write=False)
    counts = ref.counts.copy()
    counts.setflags(write=False)
    return tuple(rows), counts


def cut_ranges(nenv):
    return [(a, (nenv if b is None else b) - a) for a, b in CUTS]


@functools.lru_cache(maxsize=None)
def perm_reference(n, epoch, seed=SEED):
    walks = []
    p = dc.perm(n, epoch, seed, walks)
    p.setflags(write=False)
    return p, walks[0]


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()
