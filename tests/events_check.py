"""The event rows (phys_batch_events, include/cassie_phys.h) restated in numpy scalars and Python integers -- test infrastructure only.
The definition is the header's: per env the columns in index order, every arithmetic step one individually rounded fp64 operation
(numpy's scalar operations are), every comparison written so that a NaN takes the branch the header states.  Nothing here shares code
with the library: the device and the emulator are compared with it bit for bit."""
import numpy as np

from cassie_amd import phys as P

F64 = np.float64
ZERO, ONE = F64(0.0), F64(1.0)


class Events:
    """cols: a list of ev_* tuples (or an EV_COL_DTYPE array) with the fields as the caller writes them.  The arrays are in the host's
    shape: rows [nenv][ncols] of dtype, flags int32 [nenv], state float64 [nenv][2][ncols], words uint32 [nenv][ncols], counts uint32
    [nenv]."""

    def __init__(self, cols, nenv, dtype=np.float32, done_mask=0):
        self.cols = P.ev_cols(cols)
        self.ncols, self.nenv, self.done_mask = len(self.cols), nenv, int(done_mask)
        self.rows = np.zeros((nenv, self.ncols), dtype=dtype)
        self.flags = np.zeros(nenv, dtype=np.int32)
        self.state = np.zeros((nenv, 2, self.ncols), dtype=F64)
        self.words = np.zeros((nenv, self.ncols), dtype=np.uint32)
        self.counts = np.zeros(nenv, dtype=np.uint32)

    def _measure(self, C, row):
        with np.errstate(all="ignore"):
            e = [F64(row[int(C["index"]) + j]) - F64(C["target"]) for j in range(int(C["count"]))]
            norm = int(C["norm"])
            if norm == P.EV_SIGNED:
                return e[0]
            s = ZERO
            for x in e:
                if norm == P.EV_SUMSQ:
                    s = s + x * x
                elif norm == P.EV_SUMABS:
                    s = s + abs(x)
                else:
                    m = abs(x)
                    if m > s:
                        s = m
            return np.sqrt(s) if norm == P.EV_SUMSQ and int(C["root"]) else s

    def env(self, e, sources, reset):
        """One call on env e.  sources: {field: array [nenv][dim]} (floats are widened exactly)."""
        count = int(self.counts[e])
        fresh = count == 0 or bool(reset)
        out = [None] * self.ncols
        on = lambda k: bool(out[k] > 0.0)
        with np.errstate(all="ignore"):
            for c in range(self.ncols):
                C = self.cols[c]
                kind = int(C["kind"])
                src, trig, clear, gate = (int(C[k]) for k in ("src", "trig", "clear", "gate"))
                if kind == P.EV_MEASURE:
                    v = self._measure(C, sources[int(C["field"])][e])
                elif kind == P.EV_LEVEL:
                    w = -out[src] if int(C["sense"]) < 0 else out[src]
                    s = bool(self.words[e, c])
                    s = bool(w > C["off_thr"]) if (s and not fresh) else bool(w >= C["on_thr"])
                    self.words[e, c] = int(s)
                    v = ONE if s else ZERO
                elif kind == P.EV_TIMER:
                    t = 0 if fresh else int(self.words[e, c])
                    if on(src) != (int(C["polarity"]) == 0):
                        t = t if t == 0xFFFFFFFF else t + 1
                    else:
                        t = 0
                    self.words[e, c] = t
                    v = F64(C["dt"]) * F64(t)
                elif kind == P.EV_EDGE:
                    cur = on(src)
                    p = cur if fresh else bool(self.words[e, c])
                    op = int(C["op"])
                    hit = (cur and not p) if op == P.EV_RISING else (not cur and p) if op == P.EV_FALLING else (cur != p)
                    self.words[e, c] = int(cur)
                    v = ONE if hit else ZERO
                elif kind == P.EV_LATCH:
                    h, q = (ZERO, ZERO) if fresh else (F64(self.state[e, 0, c]), F64(self.state[e, 1, c]))
                    if on(trig):
                        h = F64(C["offset"]) + F64(C["scale"]) * (q if int(C["lag"]) else out[src])
                    v = h if (int(C["keep"]) or on(trig)) else ZERO
                    self.state[e, 0, c], self.state[e, 1, c] = h, out[src]
                elif kind == P.EV_ACCUM:
                    x = out[src]
                    m = F64(C["init"]) if (fresh or (clear >= 0 and on(clear))) else F64(self.state[e, 0, c])
                    if gate < 0 or on(gate):
                        op = int(C["op"])
                        if op == P.EV_MAX:
                            m = x if x > m else m
                        elif op == P.EV_MIN:
                            m = x if x < m else m
                        else:
                            m = m + x
                    self.state[e, 0, c] = m
                    v = m
                else:
                    assert kind == P.EV_LOGIC
                    mask = int(C["mask"])
                    members = [k for k in range(64) if (mask >> k) & 1]
                    assert members and max(members) < c
                    k = sum(1 for j in members if on(j))
                    op = int(C["op"])
                    v = F64(k) if op == P.EV_COUNT else (ONE if {P.EV_ANY: k > 0, P.EV_ALL: k == len(members), P.EV_NONE: k == 0}[op] else ZERO)
                out[c] = F64(v)
                self.rows[e, c] = out[c]     # (numpy's cast to float32 rounds to nearest even)
        self.flags[e] = int(any(on(c) for c in range(self.ncols) if (self.done_mask >> c) & 1))
        self.counts[e] = (count + 1) & 0xFFFFFFFF
        return out

    def events(self, sources, env0=0, n=None, reset=None):
        n = self.nenv - env0 if n is None else n
        for i in range(n):
            self.env(env0 + i, sources, reset is not None and reset[i] != 0)
