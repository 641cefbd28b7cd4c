"""The cases of tests/test_rays.py (the emulated ray kernel) and tests/test_rays_gpu.py (the device): tables of rays spread over the
bodies of a model and the states they are cast in -- test infrastructure only."""
import numpy as np

import depth_check as dc
import depth_scene_check as sc
import rays_check as rc
import terrain_check as tc
from test_terrain import _quat_mul, _random_quat

RMIN, RMAX = 0.03, 4.0
NRAYS = 96                    # two blocks of 64, the second half empty


def hinge_qpos(pod, qpos, rng, spread=0.35):
    """Every limited hinge of every env drawn about its start value, over `spread` of its range."""
    for j in range(pod.njnt):
        if pod.jnt_type[j] == 3 and pod.jnt_limited[j]:
            lo, hi = pod.jnt_range[j]
            a = pod.jnt_qposadr[j]
            qpos[:, a] = np.clip(qpos[:, a] + spread * (hi - lo) * rng.uniform(-0.5, 0.5, qpos.shape[0]), lo, hi)
    return qpos


def feet(pod):
    """The two bodies that carry the toe capsules (radius 0.02, half-length 0.08)."""
    out = [pod.geom_bodyid[g] for g in range(pod.ngeom) if pod.geom_type[g] == sc.CAPSULE and abs(pod.geom_size[g][0] - 0.02) < 1e-9]
    assert len(out) == 2
    return out


def aimed_table(pod, xpos0, xquat0, nrays, seed, bodies=None):
    """`nrays` rays over at least six bodies, the world included, in all three frames.  A third are probes straight down (WORLD_DIR) from
    the feet and the other bodies; a third are aimed, in the nominal pose xpos0 / xquat0 [nbody][3 / 4], from one body at a geom of
    another body (so that the robot's own solids are met); the rest leave in any direction."""
    rng = np.random.default_rng(seed)
    moving = [g for g in range(pod.ngeom) if sc.is_moving(pod, g)]
    if bodies is None:
        bodies = [0, pod.root_body[0]] + feet(pod) + sorted({pod.geom_bodyid[g] for g in moving} - set(feet(pod)) - {pod.root_body[0]})[:5]
    assert len(set(bodies)) >= 6 and 0 in bodies
    R0 = tc.quat2mat(xquat0)
    gp, gq = tc.model_geom_poses(pod, 1)
    rays = []
    for k in range(nrays):
        body = bodies[k % len(bodies)]
        kind = (k // len(bodies)) % 3
        origin = rng.uniform(-0.12, 0.12, 3)
        if body == 0:                                                   # a sensor fixed in the scene, a metre or so up, near where the robots are
            origin = np.array([rng.uniform(-2, 2), rng.uniform(-2, 2), rng.uniform(0.8, 1.8)])
        if kind == 0:
            rays.append((body, rc.WORLD_DIR, origin, [0.0, 0.0, -1.0 - rng.uniform(0, 2)]))          # (not unit: configure normalises)
        elif kind == 1 and body != 0:
            g = moving[int(rng.integers(len(moving)))]
            B = pod.geom_bodyid[g]
            target = xpos0[B] + R0[B] @ gp[0, g] + rng.uniform(-0.03, 0.03, 3)
            frame = rc.BODY if k % 2 else rc.HEADING
            Rf = R0[body] if frame == rc.BODY else rc.heading_matrix(xquat0[body])
            ow = xpos0[body] + Rf @ origin
            rays.append((body, frame, origin, Rf.T @ (target - ow)))
        else:
            d = rng.normal(size=3)
            d[2] = -abs(d[2]) if k % 2 else d[2]
            rays.append((body, (rc.BODY, rc.HEADING, rc.WORLD_DIR)[k % 3], origin, d * rng.uniform(0.5, 2.0)))
    t = rc.table_of(rays)
    assert len(set(t["frame"])) == 3 and len(set(t["body"])) >= 6
    return t


def robot_case(model, nenv, seed, stairs=None):
    """The model's start state with the pelvis anywhere over the ground at some tilt, the hinges drawn about their start values, the
    floor tilted per env, the capsules of env 2 with a pose of their own; stairs: test_terrain.stairs_case's boxes under the robot too.
    -> dict(pod, qpos, gp, gq); the body poses come from a forward pass on qpos."""
    pod = model.pod
    rng = np.random.default_rng(seed)
    if stairs is not None:
        c = stairs(model, nenv, seed)
        qpos, gp, gq = c["qpos"], c["gp"], c["gq"]
        qpos[:, 2] = rng.uniform(1.5, 1.9, nenv)                        # (the feet above the boxes, whose tops lie at up to 0.5 m)
    else:
        qpos = np.tile(model.qpos_init(), (nenv, 1))
        qpos[:, 0:2] = rng.uniform(-2, 2, (nenv, 2))
        qpos[:, 2] = rng.uniform(0.9, 1.3, nenv)
        qpos[:, 3:7] = _random_quat(rng, nenv, 0.3)
        gp, gq = tc.model_geom_poses(pod, nenv)
        floor = [g for g, t in tc.static_geoms(pod) if t == tc.PLANE][0]
        gq[:, floor] = _random_quat(rng, nenv, 0.15)
    hinge_qpos(pod, qpos, rng)
    caps = [g for g in range(pod.ngeom) if pod.geom_type[g] == sc.CAPSULE]
    gp[2, caps] += rng.uniform(-0.03, 0.03, (len(caps), 3))
    q = rng.normal(size=(len(caps), 4)) * 0.1 + [1.0, 0.0, 0.0, 0.0]
    gq[2, caps] = _quat_mul(q / np.linalg.norm(q, axis=1, keepdims=True), gq[2, caps])
    return dict(pod=pod, qpos=qpos, gp=gp, gq=gq)


def hfield_case(hf, nenv, seed, nbank=3):
    """cassie_hfield on a bank of three terrains with per-env indices; the height-field geom shifted per env and tilted in half of them."""
    pod = hf.pod
    rng = np.random.default_rng(seed)
    bank = dc.ramp_noise_flat_bank(pod.hfield_nrow, pod.hfield_ncol, nbank, seed=seed)
    index = rng.integers(0, nbank, nenv).astype(np.int32)
    index[:nbank] = np.arange(nbank)
    sx = pod.hfield_size[0]
    qpos = np.tile(hf.qpos_init(), (nenv, 1))
    qpos[:, 0:2] = rng.uniform(-0.7 * sx, 0.7 * sx, (nenv, 2))
    qpos[: max(1, nenv // 8), 0] = sx + rng.uniform(-0.3, 0.3, max(1, nenv // 8))                  # the edge, in and out
    qpos[:, 2] = rng.uniform(0.95, 1.3, nenv)
    qpos[:, 3:7] = _random_quat(rng, nenv, 0.25)
    hinge_qpos(pod, qpos, rng)
    gp, gq = tc.model_geom_poses(pod, nenv)
    g = pod.hfield_geom
    gp[:, g] += np.concatenate([rng.uniform(-0.3, 0.3, (nenv, 2)), rng.uniform(-0.1, 0.1, (nenv, 1))], axis=1)
    gq[0::2, g] = _random_quat(rng, (nenv + 1) // 2, 0.2)
    return dict(pod=pod, bank=bank, index=index, qpos=qpos, gp=gp, gq=gq)


def foot_probe_table(pod, nfan=32, nprobe=32):
    """Downward WORLD_DIR probes from both feet (a line of origins along the toe) and a forward fan in the pelvis' heading frame."""
    rays = []
    for k in range(nprobe):
        rays.append((feet(pod)[k % 2], rc.WORLD_DIR, [0.0, -0.08 + 0.16 * (k // 2) / max(1, nprobe // 2 - 1), 0.0], [0.0, 0.0, -1.0]))
    for k in range(nfan):
        a = np.radians(-60 + 120 * k / max(1, nfan - 1))
        rays.append((pod.root_body[0], rc.HEADING, [0.1, 0.0, 0.0], [np.cos(a), np.sin(a), -0.45]))
    return rc.table_of(rays)
