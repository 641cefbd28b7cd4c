"""The normaliser cases the CPU tests (tests/test_norm.py: the wave emulator) and the GPU tests (tests/test_norm_gpu.py: the device) share,
each against the restatement (tests/norm_check.py) -- test infrastructure only.  A case is a padded steps x rows tensor of D float32
columns whose padding words hold NaN, three data sets for three updates in a row, and the columns and rows that are special."""
import functools

import numpy as np

import norm_check as nc

F32, F64 = np.float32, np.float64
EPS = 1e-8
DIMS = (5, 67, 130, 340, 512)            # 340 and 512 are multiples of 4: the 16-byte path (340: 85 lanes of 16 bytes, the second group of 64 part full)
BLOCKS = (64, 16, 4096)                  # steps 3, rows 50: three blocks with the last short and one astride a step; ten blocks; one block
COL_CONST, COL_HUGE, COL_DEAD = 0, 1, 2  # a constant column, a column of +-3e38, a column that is never finite
ROW_NAN = 7                              # an env whose every word is NaN


def aligned(words, shift=0):
    """A float32 array of `words` words that begins `shift` words behind a 16-byte boundary."""
    raw = np.empty(words + 8, dtype=F32)
    at = (-(raw.ctypes.data // 4)) % 4 + shift
    return raw[at: at + words]


class Source:
    """A padded tensor: sample step * rows + row at word step * step_stride + row * row_stride of buf (NaN between the rows and steps)."""

    def __init__(self, D, steps, rows, shift=0):
        pad = 4 if D % 4 == 0 else 3     # (the 16-byte path needs strides that are multiples of 4 words)
        self.D, self.steps, self.rows = D, steps, rows
        self.row_stride = D + pad
        self.step_stride = rows * self.row_stride + 2 * pad
        self.buf = aligned(steps * self.step_stride, shift)
        self.buf[:] = np.nan

    def view(self):
        return np.lib.stride_tricks.as_strided(self.buf, shape=(self.steps, self.rows, self.D), strides=(4 * self.step_stride, 4 * self.row_stride, 4))

    def fill(self, x):
        self.buf[:] = np.nan
        self.view()[:] = x

    def dense(self):
        return np.ascontiguousarray(self.view()).reshape(self.steps * self.rows, self.D)

    def bind_args(self):
        return (self.buf.ctypes.data, self.steps, self.rows, self.step_stride, self.row_stride)


def data(D, steps, rows, seed):
    """float32 [steps][rows][D]: columns of different scale and offset; NaN, +inf and -inf scattered; the special columns and the NaN env."""
    rng = np.random.default_rng(1000 * seed + D)
    x = (rng.normal(size=(steps, rows, D)) * rng.uniform(0.01, 30.0, size=D) + rng.uniform(-50.0, 50.0, size=D)).astype(F32)
    hit = rng.random(size=x.shape) < 0.02
    x[hit] = rng.choice(np.array([np.nan, np.inf, -np.inf], dtype=F32), size=int(hit.sum()))
    x[:, :, COL_CONST] = F32(1.25)
    x[:, :, COL_HUGE] = np.where(rng.random(size=(steps, rows)) < 0.5, F32(3e38), F32(-3e38))
    x[:, :, COL_DEAD] = rng.choice(np.array([np.nan, np.inf, -np.inf], dtype=F32), size=(steps, rows))
    if rows > ROW_NAN:
        x[:, ROW_NAN, :] = np.nan
    return x


@functools.lru_cache(maxsize=None)
def datasets(D, steps, rows):
    """The data of three updates in a row: made once, shared by the tests, never changed."""
    sets = tuple(data(D, steps, rows, seed) for seed in (1, 2, 3))
    for x in sets:
        x.setflags(write=False)
    return sets


class Ref:
    """A run of the restatement in the snapshot form of norm_emu_py.Norm."""

    def __init__(self, D, block, eps=EPS, fill=0.5):
        self.D, self.block, self.eps = D, block, eps
        self.st = nc.State(D)
        self.mean, self.inv = np.full(D, fill, dtype=F32), np.full(D, fill, dtype=F32)
        self.last, self.R, self.calls = None, 0, 0

    def update(self, x):
        x = np.asarray(x, dtype=F32).reshape(-1, self.D)
        self.last, self.R, self.calls = nc.update(x, self.st, self.block, self.eps, self.mean, self.inv), len(x), self.calls + 1
        return self.snapshot()

    def write(self):
        nc.write(self.st, self.eps, self.mean, self.inv)

    def snapshot(self):
        snap = dict(zip(nc.State.NAMES, (a.copy() for a in self.st.arrays())))
        snap.update(out_mean=self.mean.copy(), out_inv=self.inv.copy(), stats=nc.stats(self.st, self.last, self.R, self.block, self.calls))
        snap.update({k: np.array(v) for k, v in self.last.items()})
        return snap


KEYS = nc.State.NAMES + ("out_mean", "out_inv", "mb", "counts", "a1", "a2", "stats")


def differing(got, want, keys=KEYS):
    """The names of what differs in a bit (a NaN equal to any NaN); empty: bit for bit the same."""
    return [k for k in keys if np.shape(got[k]) != np.shape(want[k]) or not nc.same_bits(np.asarray(got[k]), np.asarray(want[k]))]
