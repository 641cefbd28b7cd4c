"""The action rows (phys_batch_act, include/cassie_phys.h) restated in numpy and Python integers -- test infrastructure only.  The
definition is the header's: per env and column the clip, the noise (Philox4x32-10 on (env_base + env, column, counts[env], 1)), the delay
line, the low-pass, the affine map onto a base, the clip of the result, the store and the three frames of the row; every arithmetic step
one individually rounded fp64 operation (numpy's scalar operations are).  Nothing here shares code with the library but the Philox
restatement of tests/obs_check.py: the device and the emulator are compared with it bit for bit."""
import numpy as np

from cassie_amd import phys as P
from obs_check import MASK, philox4x32_10, uniform

F64 = np.float64


def noise_word(seed, env_base, env, column, count):
    return philox4x32_10(((env_base + env) & MASK, column, int(count) & MASK, 1), (seed & MASK, (seed >> 32) & MASK))[0]


def clamp(x, lo, hi):
    """clampd: a NaN passes."""
    return lo if x < lo else (hi if x > hi else x)


class Actions:
    """The rows [nenv][3][ncols], the state [nenv][D + 3][ncols] (the line's slots, newest first | f | the previous u) and the counts
    [nenv] of a configuration, advanced as phys_batch_act advances them."""

    def __init__(self, cols, nenv, delay_max=0, dtype=np.float32, seed=0, env_base=0, delay=None):
        self.cols = [{k: (int(c[k]) if k in ("bfield", "bindex", "dfield", "dindex") else F64(c[k])) for k in P.ACT_COL_DTYPE.names} for c in P.act_cols(cols)]
        self.ncols, self.D, self.seed, self.env_base = len(self.cols), int(delay_max), int(seed), int(env_base)
        self.delay = np.zeros(nenv, dtype=np.int64) if delay is None else np.asarray(delay, dtype=np.int64)
        self.rows = np.zeros((nenv, 3, self.ncols), dtype=dtype)
        self.state = np.zeros((nenv, self.D + 3, self.ncols), dtype=np.float64)
        self.counts = np.zeros(nenv, dtype=np.uint32)

    def act(self, actions, fields, env0=0, n=None, reset=None):
        """actions [nenv][>= ncols] float32 / float64; fields {field id or P.ACT_INPUT: array [nenv][dim]}: the sources are read and the
        destination elements written in place."""
        n = len(self.counts) - env0 if n is None else n
        D = self.D
        with np.errstate(all="ignore"):
            for i in range(n):
                env = env0 + i
                k = int(self.counts[env])
                fresh = k == 0 or (reset is not None and reset[i] != 0)
                d = min(max(int(self.delay[env]), 0), D)
                st = self.state[env]
                for c, col in enumerate(self.cols):
                    a = F64(actions[env, c])                  # (float32 actions widen exactly)
                    u = clamp(a, col["lo"], col["hi"])
                    v = u
                    if col["noise"] != 0:
                        v = u + col["noise"] * uniform(noise_word(self.seed, self.env_base, env, c, k))
                    if fresh:
                        st[: D + 1, c] = v
                    else:
                        for h in range(D, 0, -1):
                            st[h, c] = st[h - 1, c]
                        st[0, c] = v
                    z = F64(st[d, c])
                    f = F64(st[D + 1, c])
                    y = z if (fresh or col["smooth"] == 1) else f + col["smooth"] * (z - f)
                    st[D + 1, c] = y
                    base = col["offset"] if col["bfield"] == P.ACT_CONST else col["offset"] + F64(fields[col["bfield"]][env, col["bindex"]])
                    t = clamp(base + col["scale"] * y, col["out_lo"], col["out_hi"])
                    if col["dfield"] != P.ACT_NONE:
                        fields[col["dfield"]][env, col["dindex"]] = t
                    prev = u if fresh else F64(st[D + 2, c])
                    st[D + 2, c] = u
                    self.rows[env, :, c] = np.array([u, prev, y], dtype=np.float64).astype(self.rows.dtype)     # (round to nearest even)
                self.counts[env] = (k + 1) & MASK
        return self.rows
