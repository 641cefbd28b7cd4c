"""The height scan (phys_batch_height_scan, include/cassie_phys.h) restated in numpy FROM ITS DEFINITION, not from the kernel's text --
test infrastructure shared by tests/test_terrain.py (the emulated kernel) and tests/test_terrain_gpu.py (the device).

Definition.  Point j of the pattern, given in the heading frame of the body (origin at the body's world x, y; turned about world z by
yaw = atan2(2 (w z + x y), 1 - 2 (y y + z z)) of the body's world quaternion), is the world point (X, Y).  S(X, Y) is the highest
point at which the vertical line through it meets a static collision geom: a plane whose normal has a positive z (the intersection), a
box in any pose (here: the line against each of the six face planes, kept where it lies within the face; the kernel runs a slab test),
the height field (here: barycentric interpolation over explicitly built triangles v00 v10 v01 / v11 v01 v10 of the grid scaled by
hfield_size, in the geom's translated and yawed frame; a miss outside the footprint; a TILTED height-field geom is left out).  The
value is clamp(z_body - S, -range, +range), +range where the line meets nothing.

Besides the values, scan() says which points lie within EPS = 1e-9 m of a place where either side is right (a triangle's edge, a cell
border, the footprint's edge, a box's edge: anything that changes which surface piece the line meets): the piece under the point is
compared with the pieces under the four corners (X +- EPS, Y +- EPS) -- a border that passes within EPS of the point separates them.
"""
import numpy as np

PLANE, HFIELD, BOX = 0, 1, 6
EPS = 1e-9


def quat2mat(q):
    """[..., 4] unit quaternions (w, x, y, z) -> [..., 3, 3]."""
    w, x, y, z = (q[..., k] for k in range(4))
    R = np.empty(q.shape[:-1] + (3, 3))
    R[..., 0, 0] = w * w + x * x - y * y - z * z
    R[..., 0, 1] = 2 * (x * y - w * z)
    R[..., 0, 2] = 2 * (x * z + w * y)
    R[..., 1, 0] = 2 * (x * y + w * z)
    R[..., 1, 1] = w * w - x * x + y * y - z * z
    R[..., 1, 2] = 2 * (y * z - w * x)
    R[..., 2, 0] = 2 * (x * z - w * y)
    R[..., 2, 1] = 2 * (y * z + w * x)
    R[..., 2, 2] = w * w - x * x - y * y + z * z
    return R


def pelvis_pose(qpos):
    """World position and unit quaternion of Cassie's pelvis: three slides along the world axes and a ball joint, qpos[0:7]."""
    q = qpos[:, 3:7] / np.linalg.norm(qpos[:, 3:7], axis=1, keepdims=True)
    return qpos[:, 0:3].copy(), q


def yaw_of(quat):
    w, x, y, z = (quat[:, k] for k in range(4))
    return np.arctan2(2 * (w * z + x * y), 1 - 2 * (y * y + z * z))


def world_points(pos, quat, offsets):
    """[E][P] world X, Y of the pattern's points."""
    a = yaw_of(quat)[:, None]
    ox, oy = offsets[None, :, 0], offsets[None, :, 1]
    return pos[:, 0:1] + np.cos(a) * ox - np.sin(a) * oy, pos[:, 1:2] + np.sin(a) * ox + np.cos(a) * oy


def static_geoms(pod):
    """(geom, type) of the scanned geoms: on a body welded to the world, plane / box / height field.  (The in-scope models hold them on
    the world body or on a static body with the identity pose; asserted.)"""
    out = []
    for g in range(pod.ngeom):
        b = pod.geom_bodyid[g]
        if pod.body_weldid[b] != 0 or pod.geom_type[g] not in (PLANE, HFIELD, BOX):
            continue
        while b > 0:
            assert list(pod.body_pos[b]) == [0, 0, 0] and list(pod.body_quat[b]) == [1, 0, 0, 0], "a static body with a pose of its own"
            b = pod.body_parentid[b]
        out.append((g, pod.geom_type[g]))
    return out


def model_geom_poses(pod, nenv):
    """The model's own geom poses for every env: [nenv][ngeom][3], [nenv][ngeom][4] (what CM_P_GEOM_POS / QUAT start from)."""
    gp = np.array([list(pod.geom_pos[g]) for g in range(pod.ngeom)])
    gq = np.array([list(pod.geom_quat[g]) for g in range(pod.ngeom)])
    return np.tile(gp, (nenv, 1, 1)), np.tile(gq, (nenv, 1, 1))


def _plane(X, Y, p, R):
    """-> z [E][P], hit [E][P], piece id"""
    n = R[:, :, 2]
    ok = n[:, 2] > 0
    nz = np.where(ok, n[:, 2], 1.0)
    z = p[:, 2:3] - (n[:, 0:1] * (X - p[:, 0:1]) + n[:, 1:2] * (Y - p[:, 1:2])) / nz[:, None]
    hit = np.broadcast_to(ok[:, None], X.shape)
    return z, hit, np.zeros(X.shape, dtype=np.int64)


def _box(X, Y, p, R, size):
    """The vertical line against the six face planes; a face counts where the point lies within it."""
    best = np.full(X.shape, -np.inf)
    piece = np.zeros(X.shape, dtype=np.int64)
    for k in range(3):
        m1, m2 = (k + 1) % 3, (k + 2) % 3
        n = R[:, :, k]
        for sgn in (-1.0, 1.0):
            c = p + sgn * size[k] * n                                   # [E][3] centre of the face
            steep = n[:, 2] != 0
            nz = np.where(steep, n[:, 2], 1.0)
            z = c[:, 2:3] + (n[:, 0:1] * (c[:, 0:1] - X) + n[:, 1:2] * (c[:, 1:2] - Y)) / nz[:, None]
            d = np.stack([X - p[:, 0:1], Y - p[:, 1:2], z - p[:, 2:3]], axis=-1)          # [E][P][3]
            l1 = np.einsum("epi,ei->ep", d, R[:, :, m1])
            l2 = np.einsum("epi,ei->ep", d, R[:, :, m2])
            on = steep[:, None] & (np.abs(l1) <= size[m1]) & (np.abs(l2) <= size[m2])
            best = np.where(on & (z > best), z, best)
            piece = piece * 2 + on
    hit = np.isfinite(best)
    return np.where(hit, best, 0.0), hit, piece


def _bary(px, py, a, b, c):
    """z of the plane through the triangle's vertices a, b, c ([...][3] each) at (px, py), by barycentric coordinates."""
    det = (b[..., 1] - c[..., 1]) * (a[..., 0] - c[..., 0]) + (c[..., 0] - b[..., 0]) * (a[..., 1] - c[..., 1])
    la = ((b[..., 1] - c[..., 1]) * (px - c[..., 0]) + (c[..., 0] - b[..., 0]) * (py - c[..., 1])) / det
    lb = ((c[..., 1] - a[..., 1]) * (px - c[..., 0]) + (a[..., 0] - c[..., 0]) * (py - c[..., 1])) / det
    return la * a[..., 2] + lb * b[..., 2] + (1 - la - lb) * c[..., 2]


def _hfield(X, Y, p, R, pod, grids):
    """grids: [E][nrow][ncol] float (or None: no samples, a miss).  -> z, hit, piece, tilted [E]"""
    tilted = ~((np.abs(R[:, 0, 2]) <= 1e-12) & (np.abs(R[:, 1, 2]) <= 1e-12) & (R[:, 2, 2] > 0))
    if grids is None:
        return np.zeros(X.shape), np.zeros(X.shape, dtype=bool), np.zeros(X.shape, dtype=np.int64), tilted
    sx, sy, sz = pod.hfield_size[0], pod.hfield_size[1], pod.hfield_size[2]
    nr, nc = pod.hfield_nrow, pod.hfield_ncol
    dx, dy = X - p[:, 0:1], Y - p[:, 1:2]
    xl = R[:, 0, 0][:, None] * dx + R[:, 1, 0][:, None] * dy
    yl = R[:, 0, 1][:, None] * dx + R[:, 1, 1][:, None] * dy
    inside = (np.abs(xl) <= sx) & (np.abs(yl) <= sy) & ~tilted[:, None]
    cx, cy = 2 * sx / (nc - 1), 2 * sy / (nr - 1)
    j = np.clip(np.floor((xl + sx) / cx).astype(np.int64), 0, nc - 2)
    i = np.clip(np.floor((yl + sy) / cy).astype(np.int64), 0, nr - 2)
    e = np.arange(X.shape[0])[:, None]
    G = np.asarray(grids, dtype=np.float64)
    x0, y0 = -sx + j * cx, -sy + i * cy
    v = lambda ii, jj, xx, yy: np.stack([xx, yy, sz * G[e, ii, jj]], axis=-1)
    v00, v10, v01, v11 = v(i, j, x0, y0), v(i, j + 1, x0 + cx, y0), v(i + 1, j, x0, y0 + cy), v(i + 1, j + 1, x0 + cx, y0 + cy)
    # the diagonal v10 - v01 splits the cell: (v00, v10, v01) on the v00 side, (v11, v01, v10) on the other
    side = (xl - v10[..., 0]) * (v01[..., 1] - v10[..., 1]) - (yl - v10[..., 1]) * (v01[..., 0] - v10[..., 0])
    lower = side <= 0
    h = np.where(lower, _bary(xl, yl, v00, v10, v01), _bary(xl, yl, v11, v01, v10))
    piece = np.where(inside, 1 + 2 * (i * nc + j) + (~lower), 0)
    return p[:, 2:3] + h, inside, piece, tilted


def surface(pod, X, Y, geom_pos, geom_quat, grids):
    """S(X, Y) for [E][P] world points -> (top [E][P], hit [E][P], pieces [E][P][ngeoms scanned], tilted [E])."""
    top = np.full(X.shape, -np.inf)
    pieces = []
    tilted = np.zeros(X.shape[0], dtype=bool)
    for g, t in static_geoms(pod):
        p, R = geom_pos[:, g], quat2mat(geom_quat[:, g])
        if t == PLANE:
            z, hit, piece = _plane(X, Y, p, R)
        elif t == BOX:
            z, hit, piece = _box(X, Y, p, R, list(pod.geom_size[g]))
        else:
            z, hit, piece, tl = _hfield(X, Y, p, R, pod, grids)
            tilted |= tl
        top = np.where(hit & (z > top), z, top)
        pieces.append(np.where(hit, piece + 1, 0))
    return top, np.isfinite(top), np.stack(pieces, axis=-1), tilted


def scan(pod, qpos, offsets, scan_range, geom_pos=None, geom_quat=None, grids=None):
    """-> (values [E][P], near [E][P], tilted [E]): the scan of every env (body = the pelvis), the points that lie within EPS of a
    border between surface pieces, the envs whose height-field geom is tilted (WARN_SCAN_TILTED)."""
    qpos = np.asarray(qpos, dtype=np.float64)
    offsets = np.asarray(offsets, dtype=np.float64)
    E = qpos.shape[0]
    if geom_pos is None:
        geom_pos, geom_quat = model_geom_poses(pod, E)
    pos, quat = pelvis_pose(qpos)
    X, Y = world_points(pos, quat, offsets)
    top, hit, pieces, tilted = surface(pod, X, Y, geom_pos, geom_quat, grids)
    val = np.where(hit, np.clip(pos[:, 2:3] - np.where(hit, top, 0.0), -scan_range, scan_range), scan_range)
    near = np.zeros(X.shape, dtype=bool)
    for ex in (-EPS, EPS):
        for ey in (-EPS, EPS):
            _, _, pc, _ = surface(pod, X + ex, Y + ey, geom_pos, geom_quat, grids)
            near |= np.any(pc != pieces, axis=-1)
    return val, near, tilted


def compare(got, want, near, tol=1e-12, most_near=0.01):
    """Asserts got == want within tol wherever the point is not near a border, and that fewer than most_near of the points are."""
    frac = float(np.mean(near))
    err = np.where(near, 0.0, np.abs(got - want))
    print("height scan: %d points, %.4f %% near a border, largest difference %.3g m" % (got.size, 100 * frac, float(err.max())))
    assert frac < most_near, "%.3f %% of the points lie within 1e-9 m of a border" % (100 * frac)
    assert float(err.max()) <= tol, "differs by %.3g m at %s" % (float(err.max()), np.unravel_index(np.argmax(err), err.shape))


# ---- terrains and patterns the tests share ----
def make_bank(nrow, ncol, seed=0, count=4):
    """`count` distinct grids of elevations in [0, 1]: flat, a ramp along x, steps along y, noise, then more noise / ramps."""
    rng = np.random.default_rng(seed)
    out = []
    for k in range(count):
        kind = k % 4
        if kind == 0:
            g = np.full((nrow, ncol), 0.125 * (k // 4))
        elif kind == 1:
            g = np.tile(np.linspace(0.0, 1.0 / (1 + k // 4), ncol), (nrow, 1))
        elif kind == 2:
            g = np.tile((np.floor(np.arange(nrow) / (7 + k // 4)) % 5 / 5.0)[:, None], (1, ncol))
        else:
            g = rng.random((nrow, ncol))
        out.append(g.astype(np.float32))
    return np.stack(out)


def grid_pattern(nx=17, ny=11, step=0.1):
    """nx x ny points, `step` apart, centred a little ahead of the body: 17 x 11 = 187 points."""
    xs = (np.arange(nx) - (nx - 1) / 2) * step + 0.3
    ys = (np.arange(ny) - (ny - 1) / 2) * step
    return np.array([[x, y] for x in xs for y in ys])
