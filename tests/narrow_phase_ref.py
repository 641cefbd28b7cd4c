"""Case builders, exact references and plain-float restatements for tests/test_narrow_phase.py -- test infrastructure only.

Three kinds of function per routine of csrc/pk_collision.h:
    cases_<r>()      the trials, [n][nin] float64 in the order of the routine's arguments (the layout of the probe bodies of
                     tests/device/wave_bodies.h and of the oracle's co_test_<r>), random ones first, constructed ones after
    exact_<r>(x)     the GEOMETRIC DEFINITION evaluated on the doubles taken as exact: fractions.Fraction throughout, mpmath (50
                     digits) only where a square root is needed.  It is not the algorithm restated.
    np_<r>(x, ...)   the algorithm restated in Python floats (IEEE doubles, no contraction), with switches for the negative
                     controls' mutations
Rotation matrices are row-major with the axes in their columns.  They are orthonormal to rounding only; the references take a
box's local coordinates to be M^T (q - p) in exact arithmetic, and every bound carries the term that this costs (ORTHO)."""
import ctypes
import functools
import math
from fractions import Fraction as Fr

import mpmath
import numpy as np

mpmath.mp.dps = 50
U = 2.0 ** -53
ORTHO = 32 * U         # |M^T M - I| of a rotation matrix built below, entrywise (checked in rotations())
GR = 0.6180339887498949
WAVES = 64             # waves of 64 lane-trials per scalar routine
NBOX = 512             # wave-trials of box-box per keepmax
MPF = mpmath.mpf


# ------------------------------------------------------------------------------------------------ running things ---
def to_lanes(x):
    """[n][nin] -> [ntrial][nin][64], the last wave padded with copies of the last trial."""
    x = np.asarray(x, dtype=np.float64)
    n = x.shape[0]
    x = np.concatenate([x, np.repeat(x[-1:], -n % 64, axis=0)])
    return np.ascontiguousarray(x.reshape(-1, 64, x.shape[1]).transpose(0, 2, 1))


def run_lanes(wc, name, x):
    """A lane = trial body on the trials x[n][nin] -> [n][nout]."""
    out = wc.run(name, to_lanes(x))
    return out.transpose(0, 2, 1).reshape(-1, out.shape[1])[:len(x)]


def run_waves(wc, name, x):
    """A wave = trial body (every lane holds the trial's inputs) -> [n][nout][64]."""
    x = np.asarray(x, dtype=np.float64)
    return wc.run(name, np.ascontiguousarray(np.repeat(x[:, :, None], 64, axis=2)))


def run_oracle(name, x, nout, keep=None):
    """co_test_<name> on the trials x[n][nin] -> [n][nout] ([n][11][64] for box_box_lanes); what the routine leaves is NaN."""
    from oracle_py import lib
    x = np.ascontiguousarray(x, dtype=np.float64)
    f = getattr(lib(), "co_test_" + name)
    f.restype = None
    if keep is None:
        out = np.full((len(x), nout), np.nan)
        f.argtypes = [ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p]
        f(len(x), x.ctypes.data, out.ctypes.data)
    else:
        out = np.full((len(x), 11, 64), np.nan)
        f.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p]
        f(len(x), keep, x.ctypes.data, out.ctypes.data)
    return out


# ------------------------------------------------------------------------------------------------------ helpers ---
def fr(v):
    return [Fr(float(t)) for t in np.ravel(v)]


def fdot(a, b):
    return sum(x * y for x, y in zip(a, b))


def fsub(a, b):
    return [x - y for x, y in zip(a, b)]


def fsqrt(q):
    """Square root of a non-negative rational, 50 digits."""
    return mpmath.sqrt(MPF(q.numerator) / MPF(q.denominator))


def mp(q):
    return MPF(q.numerator) / MPF(q.denominator) if isinstance(q, Fr) else MPF(q)


def local(M, d):
    """M^T d: the coordinates of the world vector d along the columns of M."""
    return [M[0 + k] * d[0] + M[3 + k] * d[1] + M[6 + k] * d[2] for k in range(3)]


def rotations(rng, n):
    """n rotation matrices [n][9] from normalised random quaternions; |M^T M - I| <= ORTHO entrywise."""
    q = rng.normal(size=(n, 4))
    q /= np.linalg.norm(q, axis=1)[:, None]
    w, x, y, z = q.T
    M = np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y),
                  2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x),
                  2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)], axis=1)
    R = M.reshape(n, 3, 3)
    assert np.max(np.abs(np.einsum("nij,nik->njk", R, R) - np.eye(3))) <= ORTHO
    return M


def signed_permutations():
    """The 24 rotation matrices whose entries are 0 and +-1 (every operation on them is exact), [24][9]."""
    import itertools
    out = []
    for p in itertools.permutations(range(3)):
        for s in itertools.product([1.0, -1.0], repeat=3):
            M = np.zeros((3, 3))
            for i in range(3):
                M[p[i], i] = s[i]
            if np.linalg.det(M) > 0:
                out.append(M.ravel())
    return np.array(out)


def units(rng, n):
    v = rng.normal(size=(n, 3))
    return v / np.linalg.norm(v, axis=1)[:, None]


def box_sizes(rng, n):
    """Half sizes 0.005 .. 0.2, log-uniform (the tray's plate and the cube of tests/test_boxes.py lie inside)."""
    return np.exp(rng.uniform(np.log(0.005), np.log(0.2), (n, 3)))


def margins(rng, n):
    return np.where(rng.random(n) < 0.5, 0.0, 0.01)


# -------------------------------------------------------------------------------------------- plane_sphere, sphere_sphere ---
@functools.lru_cache(maxsize=None)
def cases_plane_sphere():
    rng = np.random.default_rng(701)
    n = WAVES * 64
    r = rng.uniform(0.01, 0.1, n)
    M = rotations(rng, n)
    ppos = rng.uniform(-0.5, 0.5, (n, 3))
    nrm = M[:, [2, 5, 8]]
    # centres at a height of -0.5 r .. 1.5 r + margin above the plane: both sides of dist = margin
    mg = margins(rng, n)
    hgt = r + rng.uniform(-1.5, 1.5, n) * 0.01 + mg * rng.integers(0, 2, n)
    spos = ppos + nrm * hgt[:, None] + np.cross(nrm, units(rng, n)) * rng.uniform(0, 0.3, (n, 1))
    return np.column_stack([ppos, M, spos, r, mg])


def exact_plane_sphere(x):
    """-> (dist, pos[3], scale for the bound): dist = (spos - ppos) . n - r with n the plane's third column AS GIVEN, the contact
    midway between the sphere's lowest point and the plane along n."""
    x = fr(x)
    ppos, M, spos, r = x[0:3], x[3:12], x[12:15], x[15]
    n = [M[2], M[5], M[8]]
    dif = fsub(spos, ppos)
    dist = fdot(dif, n) - r
    pos = [spos[i] - n[i] * (r + dist / 2) for i in range(3)]
    return dist, pos, float(sum(abs(a * b) for a, b in zip(dif, n)) + abs(r))


@functools.lru_cache(maxsize=None)
def cases_sphere_sphere():
    rng = np.random.default_rng(702)
    n = WAVES * 64
    r1, r2 = rng.uniform(0.01, 0.1, n), rng.uniform(0.01, 0.1, n)
    mg = margins(rng, n)
    p1 = rng.uniform(-0.5, 0.5, (n, 3))
    gap = rng.uniform(-1.5, 1.5, n) * 0.01 + mg * rng.integers(0, 2, n)
    p2 = p1 + units(rng, n) * (r1 + r2 + gap)[:, None]
    x = np.column_stack([p1, r1, p2, r2, mg])
    # constructed (exact): coincident centres, axis-aligned dyadic offsets
    tie = np.array([[0.25, -0.5, 0.125, 0.0625, 0.25, -0.5, 0.125, 0.03125, 0.0],
                    [0.25, -0.5, 0.125, 0.0625, 0.25, -0.5, 0.25, 0.0625, 0.0],
                    [0.0, 0.0, 0.0, 0.5, -0.75, 0.0, 0.0, 0.5, 0.0],
                    [0.0, 0.0, 0.0, 0.5, 0.0, 1.0, 0.0, 0.5, 0.0]])
    return np.concatenate([x, tie]), len(tie)


def exact_sphere_sphere(x):
    """-> (dist, pos, normal, centre distance) as mpf; None for the normal of coincident centres."""
    x = fr(x)
    p1, r1, p2, r2 = x[0:3], x[3], x[4:7], x[7]
    dif = fsub(p2, p1)
    cd = fsqrt(fdot(dif, dif))
    dist = cd - mp(r1) - mp(r2)
    if cd == 0:
        nrm = [MPF(1), MPF(0), MPF(0)]
    else:
        nrm = [mp(t) / cd for t in dif]
    pos = [mp(p1[i]) + nrm[i] * (mp(r1) + dist / 2) for i in range(3)]
    return dist, pos, nrm, cd


# ------------------------------------------------------------------------------------------------------ point_box ---
def exact_point_box(q, pb, M, sb, forced=None):
    """The signed distance from q to the box {|loc_k| <= sb_k}, loc = M^T (q - pb): the distance outside, minus the smallest face
    clearance inside (a point on the surface is inside, distance 0; the lowest axis on equal clearances); the outward normal in
    LOCAL axes.  All as exact rationals but the outside distance and normal (mpf).
    -> dict(inside, dist, nl, loc, e1: the margin of the inside/outside decision -- the least | |loc_k| - sb_k | over the axes
    that decide it --, e2: the gap between the two smallest clearances when inside)."""
    d = fsub(q, pb)
    loc = local(M, d)
    cl = [max(-s, min(s, t)) for t, s in zip(loc, sb)]
    inside = all(a == b for a, b in zip(cl, loc))
    over = [abs(t) - s for t, s in zip(loc, sb)]       # > 0: outside along this axis
    out = dict(loc=loc, inside=inside, l1d=sum(abs(t) for t in d))
    if inside:
        clear = [-t for t in over]
        kb = min(range(3), key=lambda k: (clear[k], k)) if forced is None else forced
        rest = sorted(clear[k] for k in range(3) if k != kb)
        out.update(dist=-clear[kb], kb=kb, nl=[(1 if loc[k] >= 0 else -1) if k == kb else 0 for k in range(3)],
                   e1=min(clear), e2=rest[0] - clear[kb])
    else:
        dif = fsub(loc, cl)
        dist = fsqrt(fdot(dif, dif))
        out.update(dist=dist, kb=-1, nl=[mp(t) / dist for t in dif], e1=max(over), e2=None)
    return out


@functools.lru_cache(maxsize=None)
def cases_point_box():
    """Random: a third well outside (faces, edges and corners), a third inside, a third within 1e-3 of the surface on either side.
    Constructed (signed-permutation frames, dyadic numbers): inside points equidistant from two and from three faces, points
    exactly on a face, an edge and a corner, the centre."""
    rng = np.random.default_rng(703)
    n = WAVES * 64
    M, sb, pb = rotations(rng, n), box_sizes(rng, n), rng.uniform(-0.3, 0.3, (n, 3))
    kind = rng.integers(0, 3, n)
    loc = np.where((kind == 0)[:, None], rng.uniform(-2.5, 2.5, (n, 3)) * sb, rng.uniform(-1, 1, (n, 3)) * sb)
    near = kind == 2
    ax = rng.integers(0, 3, n)
    sg = np.where(rng.random(n) < 0.5, -1.0, 1.0)
    loc[near, ax[near]] = (sg * (sb[np.arange(n), ax] + rng.uniform(-1e-3, 1e-3, n)))[near]
    q = pb + np.einsum("nij,nj->ni", M.reshape(n, 3, 3), loc)
    x = np.column_stack([q, pb, M, sb])
    P = signed_permutations()
    tie = []
    s = np.array([0.125, 0.25, 0.5])
    locs = [[0.0625, 0.1875, 0.0], [0.0625, -0.1875, 0.4375], [-0.0625, 0.1875, -0.4375], [0.0, 0.1875, 0.4375], [0.0, 0.0, 0.0],
            [0.125, 0.0, 0.0], [-0.125, 0.25, 0.0], [0.125, -0.25, 0.5], [0.0, 0.25, 0.25], [0.0, 0.0, -0.5], [0.0625, 0.25, -0.5],
            [0.25, 0.0, 0.0], [0.25, 0.5, 0.0], [0.25, 0.5, 1.0], [0.0, 0.0, -0.75]]
    c = np.array([0.5, -0.25, 1.0])
    for i, l in enumerate(locs):
        for Mi in (P[0], P[(5 * i + 7) % 24], P[(11 * i + 3) % 24]):
            tie.append(np.concatenate([c + Mi.reshape(3, 3) @ np.array(l), c, Mi, s]))
    return np.concatenate([x, np.array(tie)]), len(tie)


def np_point_box(q, pb, M, sb, highest=False):
    """pk_collision.h point_box in Python floats -> (dist, nworld).  highest: the negative control's mutation (ties go to the
    highest axis)."""
    d = [q[i] - pb[i] for i in range(3)]
    loc = [M[0 + k] * d[0] + M[3 + k] * d[1] + M[6 + k] * d[2] for k in range(3)]
    cl = [-sb[k] if loc[k] < -sb[k] else (sb[k] if loc[k] > sb[k] else loc[k]) for k in range(3)]
    nl = [0.0, 0.0, 0.0]
    if any(cl[k] != loc[k] for k in range(3)):
        dif = [loc[k] - cl[k] for k in range(3)]
        dist = math.sqrt(dif[0] * dif[0] + dif[1] * dif[1] + dif[2] * dif[2])
        nl = [dif[k] / dist for k in range(3)]
    else:
        best, kb = sb[0] - abs(loc[0]), 0
        for k in (1, 2):
            dk = sb[k] - abs(loc[k])
            if dk < best or (highest and dk == best):
                best, kb = dk, k
        nl[kb] = 1.0 if loc[kb] >= 0 else -1.0
        dist = -best
    return dist, [M[3 * i] * nl[0] + M[3 * i + 1] * nl[1] + M[3 * i + 2] * nl[2] for i in range(3)]


def np_sphere_box(ps, r, pb, M, sb, margin, half=True):
    """-> None or (dist, pos, normal).  half=False: the mutation that leaves the half distance out of pos."""
    d, nw = np_point_box(ps, pb, M, sb)
    dist = d - r
    if dist > margin:
        return None
    return dist, [ps[i] - nw[i] * (r + (0.5 * dist if half else 0.0)) for i in range(3)], [-t for t in nw]


@functools.lru_cache(maxsize=None)
def cases_sphere_box():
    """The points of cases_point_box as sphere centres, radii such that dist - margin falls on both sides of 0."""
    rng = np.random.default_rng(704)
    x, ntie = cases_point_box()
    n = len(x)
    mg = margins(rng, n)
    mg[n - ntie:] = 0.0
    r = rng.uniform(0.01, 0.1, n)
    r[n - ntie:] = 0.0625
    pd = np.array([np_point_box(t[0:3], t[3:6], t[6:15], t[15:18])[0] for t in x])
    # a third of the outside points: the radius that leaves a gap of -5 .. 5 mm around the margin
    pick = (rng.random(n) < 0.5) & (pd > 0.02) & (np.arange(n) < n - ntie)
    r[pick] = (pd - mg - rng.uniform(-5e-3, 5e-3, n))[pick]
    return np.column_stack([x[:, 0:3], r, x[:, 3:18], mg]), ntie


# ------------------------------------------------------------------------------------------------ segment_closest ---
@functools.lru_cache(maxsize=None)
def cases_segment_closest():
    """Random: half lengths log-uniform 0.01 .. 10, the angle between the axes such that det = 1 - (a1.a2)^2 is log-uniform over
    1e-13 .. 1 (both sides of the 1e-12 switch), centre offsets that put the closest points inside, on one end and on two ends.
    Constructed (exact): parallel and antiparallel dyadic segments -- overlapping, touching at one point, disjoint, one inside the
    other."""
    rng = np.random.default_rng(705)
    n = WAVES * 64
    a1 = units(rng, n)
    perp = np.cross(a1, units(rng, n))
    perp /= np.linalg.norm(perp, axis=1)[:, None]
    det = 10.0 ** rng.uniform(-13, 0, n)
    th = np.arcsin(np.sqrt(det)) * np.where(rng.random(n) < 0.5, 1, -1)
    flip = np.where(rng.random(n) < 0.5, 1.0, -1.0)
    a2 = flip[:, None] * (np.cos(th)[:, None] * a1 + np.sin(th)[:, None] * perp)
    a2 /= np.linalg.norm(a2, axis=1)[:, None]
    l1, l2 = 10.0 ** rng.uniform(-2, 1, n), 10.0 ** rng.uniform(-2, 1, n)
    small = rng.random(n) < 0.5
    l1[small] = rng.uniform(0.01, 0.3, n)[small]
    l2[small] = rng.uniform(0.01, 0.3, n)[small]
    third = np.cross(a1, perp)
    p1 = rng.uniform(-0.5, 0.5, (n, 3))
    p2 = p1 + a1 * (rng.uniform(-1.6, 1.6, n) * (l1 + l2))[:, None] + perp * (rng.uniform(-1.2, 1.2, n) * l2)[:, None] \
        + third * rng.uniform(0.0, 0.2, n)[:, None]
    x = np.column_stack([p1, a1, l1, p2, a2, l2])
    ex, ey = [1.0, 0.0, 0.0], [0.0, 1.0, 0.0]
    tie = []
    for s in (1.0, -1.0):
        for off, la, lb in [(0.0, 0.5, 0.25), (0.5, 0.5, 0.25), (0.75, 0.5, 0.25), (1.5, 0.5, 0.25), (-1.5, 0.5, 0.25), (0.25, 0.125, 1.0),
                            (-3.0, 0.25, 2.0), (0.0, 0.5, 0.5)]:
            tie.append([0.0, 0.0, 0.0] + ex + [la] + [off, 0.125, 0.0] + [s, 0.0, 0.0] + [lb])
    tie.append([0.0, 0.0, 0.0] + ex + [0.5] + [0.25, 0.0, 0.25] + ey + [0.5])          # crossing at right angles
    tie.append([0.0, 0.0, 0.0] + ex + [0.5] + [1.0, 2.0, 0.25] + ey + [0.5])           # both ends
    return np.concatenate([x, np.array(tie)]), len(tie)


def exact_segment_closest(x):
    """The exact minimum of f(t1, t2) = |p1 + a1 t1 - p2 - a2 t2|^2 over [-l1, l1] x [-l2, l2] (a1, a2 as given): the interior
    stationary point where the Gram determinant is not zero, the stationary point of each of the four edges, the four corners.
    -> (f min, (t1, t2) of one minimiser, whether it is the only candidate that attains the minimum, the exact Gram matrix entries)."""
    x = fr(x)
    p1, a1, l1, p2, a2, l2 = x[0:3], x[3:6], x[6], x[7:10], x[10:13], x[13]
    dif = fsub(p1, p2)
    A, B, C = fdot(a1, a1), fdot(a2, a2), fdot(a1, a2)
    D, E = fdot(a1, dif), fdot(a2, dif)

    def f(t1, t2):
        v = [dif[i] + a1[i] * t1 - a2[i] * t2 for i in range(3)]
        return fdot(v, v)
    cand = [(s1 * l1, s2 * l2) for s1 in (1, -1) for s2 in (1, -1)]
    g = A * B - C * C
    if g != 0:                                   # A t1 - C t2 = -D,  -C t1 + B t2 = E
        cand.append(((-D * B + C * E) / g, (A * E - C * D) / g))
    for t1 in (l1, -l1):
        cand.append((t1, (E + C * t1) / B))
    for t2 in (l2, -l2):
        cand.append(((-D + C * t2) / A, t2))
    cand = [(t1, t2) for t1, t2 in cand if abs(t1) <= l1 and abs(t2) <= l2]
    vals = [f(*c) for c in cand]
    fm = min(vals)
    arg = sorted(set(c for c, v in zip(cand, vals) if v == fm))
    return fm, arg[0], len(arg) == 1, f, (A, B, C, D, E)


def np_segment_closest(x, reclamp=True):
    """pk_collision.h segment_closest in Python floats.  reclamp=False: the mutation that drops the final clamp of t1."""
    p1, a1, l1, p2, a2, l2 = x[0:3], x[3:6], x[6], x[7:10], x[10:13], x[13]
    clamp = (lambda v, lo, hi: lo if v < lo else (hi if v > hi else v)) if reclamp else (lambda v, lo, hi: v)
    cl = lambda v, lo, hi: lo if v < lo else (hi if v > hi else v)
    dot = lambda a, b: a[0] * b[0] + a[1] * b[1] + a[2] * b[2]
    dif = [p1[i] - p2[i] for i in range(3)]
    mb, u, v = -dot(a1, a2), -dot(a1, dif), dot(a2, dif)
    det = 1.0 - mb * mb
    if abs(det) >= 1e-12:
        t1, t2 = (u - mb * v) / det, (v - mb * u) / det
        if t1 > l1:
            t1 = l1; t2 = v - mb * t1
        elif t1 < -l1:
            t1 = -l1; t2 = v - mb * t1
        if t2 > l2:
            t2 = l2; t1 = clamp(u - mb * t2, -l1, l1)
        elif t2 < -l2:
            t2 = -l2; t1 = clamp(u - mb * t2, -l1, l1)
    else:
        s, c2 = -mb, v
        lo, hi = max(-l2, c2 - l1), min(l2, c2 + l1)
        t2 = 0.5 * (lo + hi) if lo <= hi else cl(c2, -l2, l2)
        t1 = clamp((t2 - c2) * (1.0 if s >= 0 else -1.0), -l1, l1)
    return t1, t2


# ----------------------------------------------------------------------------------------------------- triangles ---
def cell_triangles(rng, n):
    """n grid cells: corners v00, v10, v01, v11 [n][4][3], right-angled in plan, spacings 0.02 .. 0.2, slopes from flat to 3:1."""
    dx, dy = rng.uniform(0.02, 0.2, n), rng.uniform(0.02, 0.2, n)
    x0, y0 = rng.uniform(-1, 1, n), rng.uniform(-1, 1, n)
    slope = rng.uniform(0, 3, n) * (rng.random(n) < 0.85)
    z = rng.uniform(0, 1, (n, 4)) * (slope * np.minimum(dx, dy))[:, None]
    v = np.zeros((n, 4, 3))
    v[:, :, 0] = x0[:, None] + np.array([0, 1, 0, 1]) * dx[:, None]
    v[:, :, 1] = y0[:, None] + np.array([0, 0, 1, 1]) * dy[:, None]
    v[:, :, 2] = z
    return v


def exact_closest_on_triangle(p, a, b, c):
    """The closest point of the triangle abc to p (unique, the triangle being convex): the foot of the perpendicular where it
    falls inside, else the closest point of the three edges.  Rationals throughout -> (q, squared distance)."""
    ab, ac, ap = fsub(b, a), fsub(c, a), fsub(p, a)
    g11, g12, g22 = fdot(ab, ab), fdot(ab, ac), fdot(ac, ac)
    r1, r2 = fdot(ab, ap), fdot(ac, ap)
    g = g11 * g22 - g12 * g12
    v, w = (r1 * g22 - r2 * g12) / g, (r2 * g11 - r1 * g12) / g
    best = None
    if v >= 0 and w >= 0 and v + w <= 1:
        q = [a[i] + v * ab[i] + w * ac[i] for i in range(3)]
        d = fsub(p, q)
        return q, fdot(d, d)
    for s, e in ((a, b), (a, c), (b, c)):
        se = fsub(e, s)
        t = max(Fr(0), min(Fr(1), fdot(fsub(p, s), se) / fdot(se, se)))
        q = [s[i] + t * se[i] for i in range(3)]
        d = fsub(p, q)
        dd = fdot(d, d)
        if best is None or dd < best[1]:
            best = (q, dd)
    return best


def voronoi_region(p, a, b, c):
    """0 .. 6 (the kernel's numbering: a, b, edge ab, c, edge ac, edge bc, face), exactly, for spreading the cases."""
    q, _ = exact_closest_on_triangle(p, a, b, c)
    on = [q == a, q == b, q == c]
    if on[0]: return 0
    if on[1]: return 1
    if on[2]: return 3
    ab, ac, aq = fsub(b, a), fsub(c, a), fsub(q, a)
    cr = lambda s, t: [s[1] * t[2] - s[2] * t[1], s[2] * t[0] - s[0] * t[2], s[0] * t[1] - s[1] * t[0]]
    if all(t == 0 for t in cr(ab, aq)): return 2
    if all(t == 0 for t in cr(ac, aq)): return 4
    if all(t == 0 for t in cr(fsub(c, b), fsub(q, b))): return 5
    return 6


@functools.lru_cache(maxsize=None)
def cases_triangles():
    """[n][15]: p, v00, v10, v01, v11 (closest_on_triangle takes p and the first triangle).  Lane l of every wave aims at Voronoi
    region l % 8 of the first triangle (7 = under the plane, inside the prism), so that every wave mixes all of them.
    Constructed (dyadic): points exactly on an edge, on a vertex, on the surface, and 2^-k above and below the plane around the
    1e-12 * bound switch."""
    rng = np.random.default_rng(706)
    n = WAVES * 64
    v = cell_triangles(rng, n)
    a, b, c = v[:, 0], v[:, 1], v[:, 2]
    nrm = np.cross(b - a, c - a)
    nrm /= np.linalg.norm(nrm, axis=1)[:, None]
    want = np.arange(n) % 8
    bary = np.zeros((n, 3))                     # weights of a, b, c; negative ones push the point outside across that feature
    r = rng.uniform(0.05, 0.9, (n, 3))
    far = rng.uniform(0.1, 1.5, (n, 3))
    for k in range(n):
        w = want[k]
        if w == 6 or w == 7: t = r[k] / r[k].sum()
        elif w == 0: t = [1 + far[k, 0] + far[k, 1], -far[k, 0], -far[k, 1]]
        elif w == 1: t = [-far[k, 0], 1 + far[k, 0] + far[k, 1], -far[k, 1]]
        elif w == 3: t = [-far[k, 0], -far[k, 1], 1 + far[k, 0] + far[k, 1]]
        elif w == 2: t = [r[k, 0] + far[k, 2] / 2, 1 - r[k, 0] + far[k, 2] / 2, -far[k, 2]]
        elif w == 4: t = [r[k, 0] + far[k, 2] / 2, -far[k, 2], 1 - r[k, 0] + far[k, 2] / 2]
        else: t = [-far[k, 2], r[k, 0] + far[k, 2] / 2, 1 - r[k, 0] + far[k, 2] / 2]
        bary[k] = t
    foot = bary[:, 0:1] * a + bary[:, 1:2] * b + bary[:, 2:3] * c
    h = np.where(want == 7, -rng.uniform(0.001, 0.05, n), rng.uniform(0.001, 0.1, n) * (rng.random(n) < 0.985))
    p = foot + nrm * h[:, None]
    x = np.column_stack([p, v.reshape(n, 12)])
    # constructed: the cell (0,0)-(1/4,1/4), heights 0, 1/8, 1/16, 1/4: points on vertices, on edges, on the face, around the plane
    cell = [0.0, 0.0, 0.0, 0.25, 0.0, 0.125, 0.0, 0.25, 0.0625, 0.25, 0.25, 0.25]
    A, B, C = np.array(cell[0:3]), np.array(cell[3:6]), np.array(cell[6:9])
    N = np.cross(B - A, C - A)                  # dyadic
    pts = [A, B, C, (A + B) / 2, (A + C) / 2, (B + C) / 2, (A + 3 * B) / 4, (2 * A + B + C) / 4, (A + B + 2 * C) / 4,
           A - np.array([0.5, 0.5, 0]), B + np.array([0.5, -0.25, 0])]
    on = (2 * A + B + C) / 4
    for k in (20, 30, 38, 39, 40, 41, 42, 43, 44, 46, 50, 60):
        pts += [on + N * 2.0 ** -k, on - N * 2.0 ** -k]
    flat = [0.0, 0.0, 0.0, 0.25, 0.0, 0.0, 0.0, 0.25, 0.0, 0.25, 0.25, 0.0]
    tie = [np.concatenate([pt, cell]) for pt in pts] + [np.array([0.0625, 0.0625, z] + flat) for z in (0.0, 0.5, -0.03125, 2.0 ** -45, -2.0 ** -45)]
    tie += [np.array([0.125, 0.125, 0.25] + flat), np.array([0.1875, 0.1875, 0.25] + flat), np.array([-0.25, 0.125, 0.0] + flat)]
    return np.concatenate([x, np.array(tie)]), len(tie)


def exact_hfield_cell(x):
    """The definition of the height-field contact over the two triangles of a cell (oracle/cassie_oracle.c, at `height field`): above
    a triangle's plane the distance to its closest point; below it and inside its vertical prism the signed distance to the plane;
    else the triangle does not count; the smaller of the two (the first on a tie).
    -> list per triangle of dict(kind 'above' | 'below' | 'none', s: the exact signed plane distance (mpf), snum: its numerator
    n.(p - a) with the raw normal (rational), nscale: the |n|_1 |ap|_1 the switch compares with, nrm: the unit normal, len: the
    distance to the triangle's closest point q, d = p - q, inside: p lies in the vertical prism, erel)."""
    x = fr(x)
    p, v00, v10, v01, v11 = x[0:3], x[3:6], x[6:9], x[9:12], x[12:15]
    out = []
    for a, b, c in ((v00, v10, v01), (v11, v01, v10)):
        ab, ac, ap = fsub(b, a), fsub(c, a), fsub(p, a)
        n = [ab[1] * ac[2] - ab[2] * ac[1], ab[2] * ac[0] - ab[0] * ac[2], ab[0] * ac[1] - ab[1] * ac[0]]
        if n[2] < 0:
            n = [-t for t in n]
        snum = fdot(n, ap)
        nlen = fsqrt(fdot(n, n))
        rec = dict(snum=snum, s=mp(snum) / nlen, nscale=sum(abs(t) for t in n) * sum(abs(t) for t in ap), nrm=[mp(t) / nlen for t in n])
        # both branches' quantities, whichever side of the plane p is on: a backend that decides a close call the other way is held
        # to the branch it took
        q, dd = exact_closest_on_triangle(p, a, b, c)
        e = [(s[0] - r[0]) * (p[1] - r[1]) - (s[1] - r[1]) * (p[0] - r[0]) for r, s in ((a, b), (b, c), (c, a))]
        mag = [abs((s[0] - r[0]) * (p[1] - r[1])) + abs((s[1] - r[1]) * (p[0] - r[0])) for r, s in ((a, b), (b, c), (c, a))]
        inside = all(t >= 0 for t in e) or all(t <= 0 for t in e)
        # erel: how far the closest edge function is from zero, in units of its two products' size (its rounding is 4 u of that)
        rec.update(kind="above" if snum >= 0 else ("below" if inside else "none"), inside=inside, len=fsqrt(dd), q=q, d=fsub(p, q),
                   erel=min(float(abs(t) / m) if m else 0.0 for t, m in zip(e, mag)))
        out.append(rec)
    return out


# ---------------------------------------------------------------------------------------------------- capsule_box ---
def exact_capsule_axis_minimum(pc, ax, h, pb, M, sb):
    """The exact minimum over t in [-h, h] of the signed distance from pc + ax t to the box.  The point's local coordinates are
    linear in t, so outside the box the squared distance is piecewise quadratic with break points where a coordinate meets a face
    plane, and inside the box the distance is the largest of six linear functions: the candidates are the two ends, the break
    points, the stationary point of every quadratic piece and the pairwise crossings of the linear functions.
    -> (key of the minimum, sorted list of the t that attain it, evaluate(t) -> key), key = (0, -clearance) inside,
    (1, squared distance) outside (keys order as the signed distances do)."""
    l0, l1 = local(M, fsub(pc, pb)), local(M, ax)

    def key(t):
        loc = [l0[k] + l1[k] * t for k in range(3)]
        over = [abs(loc[k]) - sb[k] for k in range(3)]
        if all(o <= 0 for o in over):
            return (0, max(over))
        return (1, sum(o * o for o in over if o > 0))
    cand = {-h, h}
    planes = [(k, s) for k in range(3) for s in (1, -1)]
    brk = sorted(set((s * sb[k] - l0[k]) / l1[k] for k, s in planes if l1[k] != 0))
    brk = [t for t in brk if -h < t < h]
    cand.update(brk)
    edges = [-h] + brk + [h]
    for lo, hi in zip(edges[:-1], edges[1:]):
        mid = (lo + hi) / 2
        loc = [l0[k] + l1[k] * mid for k in range(3)]
        act = [(k, 1 if loc[k] > 0 else -1) for k in range(3) if abs(loc[k]) > sb[k]]
        # d/dt sum (s (l0 + l1 t) - sb)^2 = 0
        den = sum(l1[k] * l1[k] for k, s in act)
        if act and den != 0:
            t = -sum(l1[k] * (l0[k] - s * sb[k]) for k, s in act) / den
            if lo <= t <= hi:
                cand.add(t)
    lin = [(s * l1[k], s * l0[k] - sb[k]) for k, s in planes]          # the six functions s loc_k - sb_k = m t + c
    for i in range(6):
        for j in range(i + 1, 6):
            dm = lin[i][0] - lin[j][0]
            if dm != 0:
                t = (lin[j][1] - lin[i][1]) / dm
                if -h <= t <= h:
                    cand.add(t)
    keys = {t: key(t) for t in cand}
    km = min(keys.values())
    return km, sorted(t for t, k in keys.items() if k == km), key


def key_dist(k):
    """The signed distance of a key, mpf."""
    return mp(k[1]) if k[0] == 0 else fsqrt(k[1])


@functools.lru_cache(maxsize=None)
def cases_capsule_box():
    """Random capsules (radius 0.01 .. 0.05, half length 0.02 .. 0.3) around random boxes: aimed at, past and through the box.
    Constructed kinds, a few hundred each, marked in `kind`: 1 the minimum at an end cap (the axis points away from the box),
    2 the axis parallel to a face (a flat minimum: distance only), 3 the axis through the box, 4 the far cap on both sides of the
    1e-6 + 1e-3 h rule (short capsules whose minimum sits 0.2 .. 5 times that far from the far end)."""
    rng = np.random.default_rng(707)
    n = WAVES * 64
    Mb, sb, pb = rotations(rng, n), box_sizes(rng, n), rng.uniform(-0.3, 0.3, (n, 3))
    Mc = rotations(rng, n)
    rad, h = rng.uniform(0.01, 0.05, n), rng.uniform(0.02, 0.3, n)
    kind = np.zeros(n, dtype=int)
    kind[: n // 2] = rng.integers(1, 5, n // 2)
    R = Mb.reshape(n, 3, 3)
    surf = rng.uniform(-1, 1, (n, 3)) * sb
    face = rng.integers(0, 3, n)
    sg = np.where(rng.random(n) < 0.5, -1.0, 1.0)
    surf[np.arange(n), face] = sg * sb[np.arange(n), face]
    out = np.zeros((n, 3)); out[np.arange(n), face] = sg                  # the face's outward normal, local
    gap = rad + rng.uniform(-0.01, 0.02, n)
    pc_loc = surf + out * gap[:, None] + rng.uniform(-0.5, 0.5, (n, 3)) * sb * (kind == 0)[:, None]
    for k in np.nonzero(kind)[0]:
        axl = None
        if kind[k] == 1:      # axis leaning away from the face by at least 20 degrees, centre one half length further out
            t = units(rng, 1)[0]; t -= out[k] * (t @ out[k]); t /= np.linalg.norm(t)
            axl = math.cos(0.8) * out[k] + math.sin(0.8) * t
            pc_loc[k] = surf[k] + out[k] * gap[k] + axl * h[k]
        elif kind[k] == 2:    # a local coordinate axis other than the face's: exactly parallel to the face
            axl = np.zeros(3); axl[(face[k] + 1 + rng.integers(0, 2)) % 3] = 1.0
            h[k] = min(h[k], 0.5 * sb[k, np.nonzero(axl)[0][0]])
            pc_loc[k] = surf[k] * 0.3 + out[k] * (sb[k, face[k]] * 0.7 + gap[k])
        elif kind[k] == 3:
            axl = units(rng, 1)[0]
            pc_loc[k] = rng.uniform(-0.8, 0.8, 3) * sb[k]
        elif kind[k] == 4:    # pointing squarely away: the minimum at the near cap t = -h; the far cap 2h away, around the rule's length
            axl = out[k]
            h[k] = rng.uniform(1e-7, 2e-6)
            pc_loc[k] = surf[k] * 0.5 + out[k] * (0.5 * sb[k, face[k]] + gap[k])
        # (the capsule's matrix: any rotation whose third column is the axis in world coordinates)
        axw = R[k] @ axl
        e = np.cross(axw, units(rng, 1)[0]); e /= np.linalg.norm(e)
        Mc[k] = np.column_stack([e, np.cross(axw, e), axw]).ravel()
    pc = pb + np.einsum("nij,nj->ni", R, pc_loc)
    return np.column_stack([pc, Mc, rad, h, pb, Mb, sb, margins(rng, n)]), kind


def np_capsule_box(x, steps=32):
    """pk_collision.h capsule_box in Python floats -> (count, ts, [contacts]).  steps: the negative control runs 16."""
    pc, mc, rad, h, pb, mb, sb, margin = x[0:3], x[3:12], x[12], x[13], x[14:17], x[17:26], x[26:29], x[29]
    ax = [mc[2], mc[5], mc[8]]
    at = lambda t: [pc[i] + ax[i] * t for i in range(3)]
    f = lambda t: np_point_box(at(t), pb, mb, sb)[0]
    lo, hi = -h, h
    t1, t2 = hi - GR * (hi - lo), lo + GR * (hi - lo)
    f1, f2 = f(t1), f(t2)
    for _ in range(steps):
        if f1 <= f2:
            hi = t2; t2 = t1; f2 = f1; t1 = hi - GR * (hi - lo); f1 = f(t1)
        else:
            lo = t1; t1 = t2; f1 = f2; t2 = lo + GR * (hi - lo); f2 = f(t2)
    ts = 0.5 * (lo + hi)
    if ts > h - 1e-9 * (1 + h): ts = h
    if ts < -h + 1e-9 * (1 + h): ts = -h
    tf = -h if ts >= 0 else h
    con = []
    c = np_sphere_box(at(ts), rad, pb, mb, sb, margin)
    if c: con.append(c)
    if not abs(tf - ts) < 1e-6 + 1e-3 * h:
        c = np_sphere_box(at(tf), rad, pb, mb, sb, margin)
        if c: con.append(c)
    return len(con), ts, con


# ------------------------------------------------------------------------------------------- make_frame, impedance ---
FRAME_MIN_HINT = 1e-6      # pk_collision.h / cassie_oracle.c: a projected hint shorter than this counts as no hint


@functools.lru_cache(maxsize=None)
def cases_make_frame():
    """[n][6] normal, hint.  Random unit normals (some of other lengths: make_frame normalises) with: no hint (both default-axis
    rules), a unit hint at a random angle, a unit hint at an angle whose sine is log-uniform over 1e-9 .. 1e-1 (both sides of
    FRAME_MIN_HINT).  Constructed: hint = +-normal exactly, for the coordinate axes and for oblique dyadic normals; normals on
    both sides of the |n_y| = 0.5 rule."""
    rng = np.random.default_rng(708)
    n = WAVES * 64
    nrm = units(rng, n)
    kind = rng.integers(0, 3, n)
    hint = units(rng, n)
    perp = np.cross(nrm, hint); perp /= np.linalg.norm(perp, axis=1)[:, None]
    sn = 10.0 ** rng.uniform(-9, -1, n)
    small = np.sqrt(1 - sn * sn)[:, None] * nrm * np.where(rng.random(n) < 0.5, -1, 1)[:, None] + sn[:, None] * perp
    small /= np.linalg.norm(small, axis=1)[:, None]
    hint = np.where((kind == 2)[:, None], small, hint)
    hint *= np.where(rng.random(n) < 0.3, rng.uniform(0.6, 3.0, n), 1.0)[:, None]      # (any length from 0.5 up is a hint)
    hint[kind == 0] = 0.0
    nrm *= np.where(rng.random(n) < 0.1, rng.uniform(0.5, 2.0, n), 1.0)[:, None]
    x = np.column_stack([nrm, hint])
    tie = []
    for v in ([1, 0, 0], [0, 1, 0], [0, 0, 1], [-1, 0, 0], [0, -1, 0], [0, 0, -1], [0.6, 0.0, 0.8], [0.0, 0.6, 0.8], [0.28, 0.96, 0.0]):
        for s in (1.0, -1.0):
            tie.append(list(v) + [s * t for t in v])
        tie.append(list(v) + [0.0, 0.0, 0.0])
    for ny in (0.5, -0.5, 0.4999999999999999, 0.5000000000000001):
        tie.append([math.sqrt(1 - ny * ny), ny, 0.0, 0.0, 0.0, 0.0])
    return np.concatenate([x, np.array(tie)]), len(tie)


def np_make_frame(x):
    dot = lambda a, b: a[0] * b[0] + a[1] * b[1] + a[2] * b[2]

    def normalize(a):
        n = math.sqrt(dot(a, a))
        if n < 1e-15:
            return [1.0, 0.0, 0.0]
        s = 1.0 / n
        return [a[0] * s, a[1] * s, a[2] * s]
    n, t = normalize(list(x[0:3])), list(x[3:6])
    hh, th = dot(t, t), dot(n, t)
    if hh < 0.25 or hh - th * th < FRAME_MIN_HINT * FRAME_MIN_HINT:
        t = [0.0, 1.0, 0.0] if -0.5 < n[1] < 0.5 else [0.0, 0.0, 1.0]
    d = dot(n, t)
    t = normalize([t[i] - d * n[i] for i in range(3)])
    return n + t + [n[1] * t[2] - n[2] * t[1], n[2] * t[0] - n[0] * t[2], n[0] * t[1] - n[1] * t[0]]


SOLIMP = (0.9, 0.95, 0.001, 0.5, 2.0)


@functools.lru_cache(maxsize=None)
def cases_impedance():
    """[n][7] solimp, pos, margin.  Random: the model's solimp and random ones (power 1 and 2), penetrations across the whole
    width.  Constructed: the values of tests/test_softness_pins.py, x exactly 0, mid and 1, dmin == dmax, width <= CM_MINVAL,
    power 1."""
    rng = np.random.default_rng(709)
    n = WAVES * 64
    imp = np.tile(SOLIMP, (n, 1))
    odd = rng.random(n) < 0.5
    imp[odd, 0] = rng.uniform(0.1, 0.9, odd.sum())
    imp[odd, 1] = rng.uniform(0.9, 0.999, odd.sum())
    imp[odd, 2] = 10.0 ** rng.uniform(-4, -1, odd.sum())
    imp[odd, 3] = rng.uniform(0.1, 0.9, odd.sum())
    imp[odd, 4] = rng.integers(1, 3, odd.sum())
    mg = margins(rng, n)
    pos = mg + rng.uniform(-1.3, 1.3, n) * imp[:, 2]
    x = np.column_stack([imp, pos, mg])
    S = list(SOLIMP)
    tie = [S + [r, 0.0] for r in (0.0, -0.002, 0.001, 0.0005, 0.00025, -0.0005, -0.001, 0.75 * 0.001)]
    D = [0.5, 0.75, 0.25, 0.5, 2.0]            # dyadic: every operation exact
    tie += [D + [r, m] for r, m in ((0.0, 0.0), (0.125, 0.0), (-0.125, 0.0), (0.25, 0.0), (-0.25, 0.0), (0.0625, 0.0), (0.1875, 0.0), (0.5, 0.0),
                                    (0.25, 0.125), (0.125, 0.125), (0.375, 0.125), (0.0, 0.125))]
    tie += [[0.5, 0.75, 0.25, 0.5, 1.0, r, 0.0] for r in (0.0, 0.0625, 0.125, 0.25, 0.375)]
    tie += [[0.75, 0.75, 0.25, 0.5, 2.0, 0.0625, 0.0], [0.5, 0.75, 1e-15, 0.5, 2.0, 0.0625, 0.0], [0.5, 0.75, 0.0, 0.5, 2.0, 0.0, 0.0],
            [0.5, 0.75, -1.0, 0.5, 2.0, 0.3, 0.0]]
    return np.concatenate([x, np.array(tie)]), len(tie)


def exact_impedance(x):
    """MuJoCo's documented sigmoid for power 1 and 2 (the exponents the model compiler admits), in rationals."""
    d0, d1, width, mid, power, pos, margin = fr(x)
    if d0 == d1 or width <= Fr(1e-15):
        return (d0 + d1) / 2
    t = abs((pos - margin) / width)
    if t >= 1:
        return d1
    if power == 1:
        y = t
    else:
        y = t * t / mid if t <= mid else 1 - (1 - t) * (1 - t) / (1 - mid)
    return d0 + y * (d1 - d0)


# --------------------------------------------------------------------------------------------------------- box-box ---
def _rot_axis(axis, ang):
    a = np.asarray(axis, dtype=float) / np.linalg.norm(axis)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + math.sin(ang) * K + (1 - math.cos(ang)) * (K @ K)


@functools.lru_cache(maxsize=None)
def cases_box_box():
    """[n][31] p1, m1, s1, p2, m2, s2, margin.  Random: box 1 anywhere; box 2 turned at random (a third), turned about box 1's
    face normal only (a third: face on face, many candidates), or tilted by up to 0.1 rad from that (a third); placed along a
    random direction or along a face normal of box 1 so that the support gap is -20 .. 12 mm, with a lateral offset.
    Constructed (signed-permutation frames, dyadic numbers), in this order:
      0 aligned equal cubes touching face to face along x, offset along no other axis: faces of A and B and nothing else tie
      1 aligned cubes overlapping by the same depth along x and y: two faces of A tie -> the lower axis
      2 two boxes of the same footprint stacked: eight equal-depth candidates (4 incident vertices, 4 rectangle corners)
      3 the same with box 2 the smaller footprint strictly inside: four incident vertices only
      4 a partial overlap whose incident vertices lie exactly on the rectangle's rim lines (sp exactly 0 or 1 is no crossing)
      5 a partial overlap, offset along both face axes
      6 box 2 turned by a quarter turn (another signed permutation), same footprint stacked
      7 separated by exactly the margin (a contact), 8 by one ulp step more in dyadic terms (none)"""
    rng = np.random.default_rng(710)
    n = NBOX
    M1, s1, p1 = rotations(rng, n), box_sizes(rng, n), rng.uniform(-0.3, 0.3, (n, 3))
    s2 = box_sizes(rng, n)
    R1 = M1.reshape(n, 3, 3)
    kind = rng.integers(0, 3, n)
    x = np.zeros((n, 31))
    for k in range(n):
        f = rng.integers(0, 3)
        if kind[k] == 0:
            R2 = rotations(rng, 1)[0].reshape(3, 3)
            dirn = units(rng, 1)[0] if rng.random() < 0.5 else R1[k][:, f] * rng.choice([-1.0, 1.0])
        else:
            P = signed_permutations()[rng.integers(0, 24)].reshape(3, 3)
            R2 = R1[k] @ _rot_axis(np.eye(3)[f], rng.uniform(0, 2 * np.pi)) @ P
            if kind[k] == 2:
                R2 = _rot_axis(units(rng, 1)[0], rng.uniform(0, 0.1)) @ R2
            dirn = R1[k][:, f] * rng.choice([-1.0, 1.0])
        ext = np.abs(R1[k].T @ dirn) @ s1[k] + np.abs(R2.T @ dirn) @ s2[k]
        lat = np.cross(dirn, units(rng, 1)[0]) * rng.uniform(0, 0.8) * min(s1[k].max(), s2[k].max())
        p2 = p1[k] + dirn * (ext + rng.uniform(-0.02, 0.012)) + lat
        x[k] = np.concatenate([p1[k], M1[k], s1[k], p2, R2.ravel(), s2[k], [0.0 if rng.random() < 0.5 else 0.01]])
    I, P = np.eye(3).ravel(), signed_permutations()
    c, h = [0.5, -0.25, 1.0], 0.125
    tie = [c + list(I) + [h, h, h] + [c[0] + 0.25, c[1], c[2]] + list(I) + [h, h, h] + [0.0],
           c + list(I) + [h, h, h] + [c[0] + 0.1875, c[1] + 0.1875, c[2]] + list(I) + [h, h, h] + [0.0],
           c + list(I) + [h, 0.25, 0.0625] + [c[0], c[1], c[2] + 0.125 - 0.0078125] + list(I) + [h, 0.25, 0.0625] + [0.0],
           c + list(I) + [h, 0.25, 0.0625] + [c[0], c[1], c[2] + 0.125 - 0.0078125] + list(I) + [0.0625, 0.125, 0.0625] + [0.0],
           c + list(I) + [h, 0.25, 0.0625] + [c[0] + 0.125, c[1], c[2] + 0.125 - 0.0078125] + list(I) + [0.25, 0.125, 0.0625] + [0.0],
           c + list(I) + [h, 0.25, 0.0625] + [c[0] + 0.0625, c[1] + 0.375, c[2] + 0.125 - 0.0078125] + list(I) + [0.125, 0.25, 0.0625] + [0.0],
           c + list(P[7]) + [h, h, h] + [c[0], c[1], c[2] + 0.25 - 0.0078125] + list(P[13]) + [h, h, h] + [0.0],
           c + list(I) + [h, h, h] + [c[0], c[1], c[2] + 0.25 + 0.0078125] + list(I) + [h, h, h] + [0.0078125],
           c + list(I) + [h, h, h] + [c[0], c[1], c[2] + 0.25 + 0.0078125 + 2.0 ** -40] + list(I) + [h, h, h] + [0.0078125]]
    return np.concatenate([x, np.array(tie)]), len(tie)


def exact_box_box(x, chosen=None):
    """The exact side of box_box_lane's definition on one case (rationals; mpf for the edge axes' lengths).
    -> dict: seps (15 exact separations, None where the edge axis does not exist: 1 - (A_i . B_j)^2 < 1e-6), scores (the same
    with the documented preferences: faces of A, faces of B less 1e-10, edges -- penetrations counted 5 % deeper -- less 2e-10),
    best (the first axis of the largest score), second (the gap to the runner-up).  With chosen = an axis 0 .. 5: the face contact
    on that reference axis -- cand: {candidate: (u, v, w)} of the vertices of the incident face clipped to the reference
    rectangle, numbered as the kernel's lanes (0-3 incident vertices inside the rectangle, 4-7 rectangle corners inside the
    projected incident face, 8 + 4 e + l incident edge e crossing rectangle line l strictly inside both), polygon: the same
    vertex set by Sutherland-Hodgman clipping (points only), slack: the least distance of any decision from its threshold
    divided by the scale it is measured in, frame: cr, Ra1, Ra2, n."""
    v = fr(x)
    p1, m1, s1, p2, m2, s2, margin = v[0:3], v[3:12], v[12:15], v[15:18], v[18:27], v[27:30], v[30]
    A = [[m1[3 * k + i] for k in range(3)] for i in range(3)]
    B = [[m2[3 * k + i] for k in range(3)] for i in range(3)]
    d = fsub(p2, p1)
    ta, tb = [fdot(d, A[i]) for i in range(3)], [fdot(d, B[i]) for i in range(3)]
    C = [[fdot(A[i], B[j]) for j in range(3)] for i in range(3)]
    Q = [[abs(t) for t in r] for r in C]
    seps, scores = [], []
    for k in range(3):
        sep = abs(ta[k]) - (s1[k] + sum(s2[j] * Q[k][j] for j in range(3)))
        seps.append(mp(sep)); scores.append(mp(sep))
    for j in range(3):
        sep = abs(tb[j]) - (s2[j] + sum(s1[i] * Q[i][j] for i in range(3)))
        seps.append(mp(sep)); scores.append(mp(sep) - MPF(1e-10))
    minlen2 = None
    for i in range(3):
        for j in range(3):
            i1, i2, j1, j2 = (i + 1) % 3, (i + 2) % 3, (j + 1) % 3, (j + 2) % 3
            len2 = 1 - C[i][j] * C[i][j]
            minlen2 = abs(len2 - Fr(1e-6)) if minlen2 is None else min(minlen2, abs(len2 - Fr(1e-6)))
            if len2 < Fr(1e-6):
                seps.append(None); scores.append(None)
                continue
            proj = ta[i2] * C[i1][j] - ta[i1] * C[i2][j]
            sep = mp(abs(proj) - (s1[i1] * Q[i2][j] + s1[i2] * Q[i1][j] + s2[j1] * Q[i][j2] + s2[j2] * Q[i][j1])) / fsqrt(len2)
            seps.append(sep); scores.append((sep * MPF(1.05) if sep < 0 else sep) - MPF(2e-10))
    order = sorted((k for k in range(15) if scores[k] is not None), key=lambda k: (-scores[k], k))
    out = dict(seps=seps, scores=scores, best=order[0], second=scores[order[0]] - scores[order[1]], maxsep=max(t for t in seps if t is not None),
               margin=margin, mmargin=mp(margin), A=A, B=B, p1=p1, p2=p2, s1=s1, s2=s2, len2band=minlen2)
    if chosen is None or chosen >= 6:
        return out
    refA, a = chosen < 3, chosen % 3
    a1, a2 = (a + 1) % 3, (a + 2) % 3
    Rm, Im = (A, B) if refA else (B, A)
    pr, pi, sr, si = (p1, p2, s1, s2) if refA else (p2, p1, s2, s1)
    dri = fsub(pi, pr)
    sgn = 1 if fdot(dri, Rm[a]) >= 0 else -1
    nrm = [sgn * t for t in Rm[a]]
    dots = [abs(fdot(nrm, Im[k])) for k in range(3)]
    kf = 0
    for k in (1, 2):
        if dots[k] > dots[kf] + Fr(1e-9):
            kf = k
    sd = sorted(dots)
    kfslack = abs(sd[2] - sd[1]) - Fr(1e-9)      # the incident face's choice: the two largest |n . I_k| against the routine's 1e-9 window
    k1, k2 = (kf + 1) % 3, (kf + 2) % 3
    isg = -1 if fdot(nrm, Im[kf]) > 0 else 1
    cr = [pr[t] + sgn * sr[a] * Rm[a][t] for t in range(3)]
    ci = [pi[t] + isg * si[kf] * Im[kf][t] for t in range(3)]
    h1, h2 = sr[a1], sr[a2]
    su, sv = [1, -1, -1, 1], [1, 1, -1, -1]
    P = []
    for q in range(4):
        xx = [ci[t] + su[q] * si[k1] * Im[k1][t] + sv[q] * si[k2] * Im[k2][t] - cr[t] for t in range(3)]
        P.append((fdot(xx, Rm[a1]), fdot(xx, Rm[a2]), fdot(xx, nrm)))
    cand, decisions = {}, []
    for q in range(4):
        decisions += [(abs(abs(P[q][0]) - h1), 1), (abs(abs(P[q][1]) - h2), 1)]
        if abs(P[q][0]) <= h1 and abs(P[q][1]) <= h2:
            cand[q] = P[q]
    e1, e2 = [P[1][t] - P[0][t] for t in range(3)], [P[3][t] - P[0][t] for t in range(3)]
    det = e1[0] * e2[1] - e1[1] * e2[0]
    for q in range(4):
        u, w_ = su[q] * h1, sv[q] * h2
        crs = [(P[(e + 1) & 3][0] - P[e][0]) * (w_ - P[e][1]) - (P[(e + 1) & 3][1] - P[e][1]) * (u - P[e][0]) for e in range(4)]
        decisions += [(abs(t), 2) for t in crs]
        if det != 0 and not (any(t > 0 for t in crs) and any(t < 0 for t in crs)):
            gu, gv = (e1[2] * e2[1] - e1[1] * e2[2]) / det, (e1[0] * e2[2] - e1[2] * e2[0]) / det
            cand[4 + q] = (u, w_, P[0][2] + gu * (u - P[0][0]) + gv * (w_ - P[0][1]))
    slope = Fr(0)
    for e in range(4):
        f = (e + 1) & 3
        for l in range(4):
            along_u = l < 2
            lim = (-1 if l & 1 else 1) * (h1 if along_u else h2)
            x0, x1 = (P[e][0], P[f][0]) if along_u else (P[e][1], P[f][1])
            y0, y1 = (P[e][1], P[f][1]) if along_u else (P[e][0], P[f][0])
            hy = h2 if along_u else h1
            dx = x1 - x0
            decisions += [(abs(lim - x0), 1), (abs(lim - x1), 1)]
            if dx == 0:
                continue
            sp = (lim - x0) / dx
            if not (0 < sp < 1):
                continue
            y = y0 + sp * (y1 - y0)
            sl = 1 + (abs(y1 - y0) + abs(P[f][2] - P[e][2])) / abs(dx)
            decisions.append((abs(abs(y) - hy) / sl, 1))
            if abs(y) > hy:
                continue
            slope = max(slope, sl)
            cand[8 + 4 * e + l] = ((lim, y) if along_u else (y, lim)) + (P[e][2] + sp * (P[f][2] - P[e][2]),)
    out.update(cand=cand, decisions=decisions, kfslack=kfslack, slope=slope, frame=(cr, Rm[a1], Rm[a2], nrm), refA=refA, rect=(h1, h2), P=P)
    return out


def clip_polygon(P, h1, h2):
    """Sutherland-Hodgman: the quadrilateral P (u, v, w per vertex) clipped to |u| <= h1, |v| <= h2 -> the set of (u, v, w)."""
    poly = list(P)
    for axis, lim, sign in ((0, h1, 1), (0, h1, -1), (1, h2, 1), (1, h2, -1)):
        nxt = []
        for i in range(len(poly)):
            a, b = poly[i], poly[(i + 1) % len(poly)]
            ina, inb = sign * a[axis] <= lim, sign * b[axis] <= lim
            if ina:
                nxt.append(a)
            if ina != inb:
                t = (sign * lim - a[axis]) / (b[axis] - a[axis])
                nxt.append(tuple(a[c] + t * (b[c] - a[c]) for c in range(3)))
        poly = nxt
        if not poly:
            break
    return set(poly)


def np_box_box(x, keepmax, sp_closed=False, lane_rank=False):
    """pk_collision.h box_box_lane's face branch in Python floats -> the sorted list of kept candidates (None for a separated pair,
    'edge' for an edge contact).  sp_closed: the mutation that counts sp == 1 as a crossing; lane_rank: ranks by lane only."""
    p1, m1, s1, p2, m2, s2, margin = x[0:3], x[3:12], x[12:15], x[15:18], x[18:27], x[27:30], x[30]
    dot = lambda a, b: a[0] * b[0] + a[1] * b[1] + a[2] * b[2]
    A = [[m1[3 * k + i] for k in range(3)] for i in range(3)]
    B = [[m2[3 * k + i] for k in range(3)] for i in range(3)]
    d = [p2[i] - p1[i] for i in range(3)]
    ta, tb = [dot(d, A[i]) for i in range(3)], [dot(d, B[i]) for i in range(3)]
    C = [[dot(A[i], B[j]) for j in range(3)] for i in range(3)]
    Q = [[abs(t) for t in r] for r in C]
    best, bestscore = -1, 0.0
    for k in range(15):
        if k < 3:
            sep = abs(ta[k]) - (s1[k] + (s2[0] * Q[k][0] + s2[1] * Q[k][1] + s2[2] * Q[k][2])); sc = sep
        elif k < 6:
            j = k - 3
            sep = abs(tb[j]) - (s2[j] + (s1[0] * Q[0][j] + s1[1] * Q[1][j] + s1[2] * Q[2][j])); sc = sep - 1e-10
        else:
            i, j = (k - 6) // 3, (k - 6) % 3
            i1, i2, j1, j2 = (i + 1) % 3, (i + 2) % 3, (j + 1) % 3, (j + 2) % 3
            len2 = 1.0 - C[i][j] * C[i][j]
            if len2 < 1e-6:
                continue
            proj = ta[i2] * C[i1][j] - ta[i1] * C[i2][j]
            sep = (abs(proj) - ((s1[i1] * Q[i2][j] + s1[i2] * Q[i1][j]) + (s2[j1] * Q[i][j2] + s2[j2] * Q[i][j1]))) / math.sqrt(len2)
            sc = (1.05 * sep if sep < 0 else sep) - 2e-10
        if sep > margin:
            return None
        if best < 0 or sc > bestscore:
            best, bestscore = k, sc
    if best >= 6:
        return "edge"
    refA, a = best < 3, best % 3
    a1, a2 = (a + 1) % 3, (a + 2) % 3
    Rm, Im = (A, B) if refA else (B, A)
    pr, pi, sr, si = (p1, p2, s1, s2) if refA else (p2, p1, s2, s1)
    dri = [pi[i] - pr[i] for i in range(3)]
    sgn = 1.0 if dot(dri, Rm[a]) >= 0 else -1.0
    n = [sgn * t for t in Rm[a]]
    kf, kbest = 0, abs(dot(n, Im[0]))
    for k in (1, 2):
        v = abs(dot(n, Im[k]))
        if v > kbest + 1e-9:
            kbest, kf = v, k
    k1, k2 = (kf + 1) % 3, (kf + 2) % 3
    isg = -1.0 if dot(n, Im[kf]) > 0 else 1.0
    cr = [pr[t] + sgn * sr[a] * Rm[a][t] for t in range(3)]
    ci = [pi[t] + isg * si[kf] * Im[kf][t] for t in range(3)]
    h1, h2 = sr[a1], sr[a2]
    su, sv = [1.0, -1.0, -1.0, 1.0], [1.0, 1.0, -1.0, -1.0]
    pu, pv, pw = [], [], []
    for q in range(4):
        xx = [ci[t] + su[q] * si[k1] * Im[k1][t] + sv[q] * si[k2] * Im[k2][t] - cr[t] for t in range(3)]
        pu.append(dot(xx, Rm[a1])); pv.append(dot(xx, Rm[a2])); pw.append(dot(xx, n))
    tol = 1e-12
    w, valid = [0.0] * 24, [False] * 24
    for q in range(4):
        w[q] = pw[q]
        valid[q] = abs(pu[q]) <= h1 + tol and abs(pv[q]) <= h2 + tol
    e1u, e1v, e1w, e2u, e2v, e2w = pu[1] - pu[0], pv[1] - pv[0], pw[1] - pw[0], pu[3] - pu[0], pv[3] - pv[0], pw[3] - pw[0]
    det = e1u * e2v - e1v * e2u
    if det != 0:
        gu, gv = (e1w * e2v - e1v * e2w) / det, (e1u * e2w - e1w * e2u) / det
        for q in range(4):
            u, v = su[q] * h1, sv[q] * h2
            pos = neg = 0
            for e in range(4):
                f = (e + 1) & 3
                c2 = (pu[f] - pu[e]) * (v - pv[e]) - (pv[f] - pv[e]) * (u - pu[e])
                pos += c2 > tol; neg += c2 < -tol
            w[4 + q] = pw[0] + gu * (u - pu[0]) + gv * (v - pv[0])
            valid[4 + q] = not (pos and neg)
    for e in range(4):
        f = (e + 1) & 3
        for l in range(4):
            along_u = l < 2
            lim = (-1 if l & 1 else 1) * (h1 if along_u else h2)
            x0, x1 = (pu[e], pu[f]) if along_u else (pv[e], pv[f])
            y0, y1 = (pv[e], pv[f]) if along_u else (pu[e], pu[f])
            dx = x1 - x0
            if abs(dx) < 1e-14:
                continue
            sp = (lim - x0) / dx
            if not (sp > 0 and (sp <= 1 if sp_closed else sp < 1)):
                continue
            y = y0 + sp * (y1 - y0)
            if abs(y) > (h2 if along_u else h1):
                continue
            w[8 + 4 * e + l] = pw[e] + sp * (pw[f] - pw[e]); valid[8 + 4 * e + l] = True
    valid = [valid[q] and not w[q] > margin for q in range(24)]
    keep = list(valid)
    if sum(valid) > keepmax:
        for q in range(24):
            if not valid[q]:
                continue
            rank = sum(1 for r in range(24) if r != q and valid[r] and ((r < q) if lane_rank else (w[r] < w[q] - 1e-9 or (abs(w[r] - w[q]) <= 1e-9 and r < q))))
            keep[q] = rank < keepmax
    return [q for q in range(24) if keep[q]]


# ------------------------------------------------------------------ plain-float restatements of the remaining routines ---
_NAN = float("nan")


def _dot(a, b):
    return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]


def _contact_row(n, dist=_NAN, pos=(_NAN,) * 3, normal=(_NAN,) * 3, tangent=(_NAN,) * 3):
    return [float(n), dist, *pos, *normal, *tangent]


def np_plane_sphere(x):
    """-> the probe body's 11 outputs (count, dist, pos, normal, tangent; NaN where nothing is written)."""
    ppos, m, spos, r, margin = x[0:3], x[3:12], x[12:15], x[15], x[16]
    n = [m[2], m[5], m[8]]
    dist = _dot([spos[i] - ppos[i] for i in range(3)], n) - r
    if dist > margin:
        return _contact_row(0)
    return _contact_row(1, dist, [spos[i] - n[i] * (r + 0.5 * dist) for i in range(3)], n, (0.0,) * 3)


def np_sphere_sphere(x):
    p1, r1, p2, r2, margin = x[0:3], x[3], x[4:7], x[7], x[8]
    dif = [p2[i] - p1[i] for i in range(3)]
    cd = math.sqrt(_dot(dif, dif))
    dist = cd - r1 - r2
    if dist > margin:
        return _contact_row(0)
    n = [1.0, 0.0, 0.0] if cd < 1e-15 else [dif[i] / cd for i in range(3)]
    return _contact_row(1, dist, [p1[i] + n[i] * (r1 + 0.5 * dist) for i in range(3)], n, (0.0,) * 3)


def np_closest_on_triangle(p, a, b, c):
    ab, ac = [b[i] - a[i] for i in range(3)], [c[i] - a[i] for i in range(3)]
    ap, bp, cp = [p[i] - a[i] for i in range(3)], [p[i] - b[i] for i in range(3)], [p[i] - c[i] for i in range(3)]
    d1, d2, d3, d4, d5, d6 = _dot(ab, ap), _dot(ac, ap), _dot(ab, bp), _dot(ac, bp), _dot(ab, cp), _dot(ac, cp)
    vc, vb, va = d1 * d4 - d3 * d2, d5 * d2 - d1 * d6, d3 * d6 - d5 * d4
    v = w = 0.0
    if d1 <= 0 and d2 <= 0: pass
    elif d3 >= 0 and d4 <= d3: v = 1.0
    elif vc <= 0 and d1 >= 0 and d3 <= 0: v = d1 / (d1 - d3)
    elif d6 >= 0 and d5 <= d6: w = 1.0
    elif vb <= 0 and d2 >= 0 and d6 <= 0: w = d2 / (d2 - d6)
    elif va <= 0 and (d4 - d3) >= 0 and (d5 - d6) >= 0:
        w = (d4 - d3) / ((d4 - d3) + (d5 - d6)); v = 1 - w
    else:
        t = 1.0 / (va + vb + vc); v = vb * t; w = vc * t
    return [a[i] + v * ab[i] + w * ac[i] for i in range(3)]


def np_hfield_cell(x):
    """The fold of hfield_triangle over the cell's two triangles -> (best, normal): the oracle's form (unit normal first)."""
    p = x[0:3]
    best, bn = 1e300, [0.0, 0.0, 1.0]
    for a, b, c in ((x[3:6], x[6:9], x[9:12]), (x[12:15], x[9:12], x[6:9])):
        ab, ac = [b[i] - a[i] for i in range(3)], [c[i] - a[i] for i in range(3)]
        n = [ab[1] * ac[2] - ab[2] * ac[1], ab[2] * ac[0] - ab[0] * ac[2], ab[0] * ac[1] - ab[1] * ac[0]]
        if n[2] < 0:
            n = [-t for t in n]
        inv = 1.0 / math.sqrt(_dot(n, n))
        n = [t * inv for t in n]
        s = _dot(n, [p[i] - a[i] for i in range(3)])
        if s >= 0:
            q = np_closest_on_triangle(p, a, b, c)
            d = [p[i] - q[i] for i in range(3)]
            ln = math.sqrt(_dot(d, d))
            if ln < best:
                best, bn = ln, ([d[i] / ln for i in range(3)] if ln > 1e-12 else n)
        else:
            e = [(s_[0] - r[0]) * (p[1] - r[1]) - (s_[1] - r[1]) * (p[0] - r[0]) for r, s_ in ((a, b), (b, c), (c, a))]
            if (all(t >= 0 for t in e) or all(t <= 0 for t in e)) and s < best:
                best, bn = s, n
    return [best] + list(bn)


def np_impedance(x):
    dmin, dmax, width, mid, power, pos, margin = x
    if dmin == dmax or width <= 1e-15:
        return 0.5 * (dmin + dmax)
    t = abs((pos - margin) / width)
    if t >= 1: return dmax
    if t <= 0: return dmin
    y = t if power == 1 else (t * t / mid if t <= mid else 1 - (1 - t) * (1 - t) / (1 - mid))
    return dmin + y * (dmax - dmin)
