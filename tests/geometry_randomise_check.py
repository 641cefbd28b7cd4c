"""Shared by the emulator and the GPU tests of per-env geometry / spring randomisation: the four inputs CM_P_GEOM_POS,
CM_P_GEOM_QUAT, CM_P_JNT_STIFFNESS, CM_P_QPOS_SPRING and what the device derives from them, against the HOST's answer -- a host
model edited through the views the reference writes (cassie_sim_set_geom_name_pos / _quat, reference src/cassiemujoco.c:1478-1537;
jnt_stiffness / qpos_spring through the raw model), then compiled.  Builds on randomise_check (the five other inputs).
Test infrastructure only."""
import ctypes

import numpy as np

import randomise_check as rc
from cassie_amd import phys as P
from cassie_amd._lib import CmEnvParams

GEO_INPUTS = ("geom_pos", "geom_quat", "jnt_stiffness", "qpos_spring")
GEO_DERIVED = ("geom_mat", "body_reach", "dof_stiffness", "dof_springref")
GEO_IDS = {"geom_pos": P.P_GEOM_POS, "geom_quat": P.P_GEOM_QUAT, "jnt_stiffness": P.P_JNT_STIFFNESS, "qpos_spring": P.P_QPOS_SPRING}
ALL_IDS = dict(rc.PARAM_IDS, **GEO_IDS)


def own_params(pod, nenv):
    """Every input of the model's own block, [nenv][dim] each (the nine fields Batch.randomize takes)."""
    a = params_as_arrays(pod.params, pod)
    b = rc.params_as_arrays(pod.params, pod)
    out = {f: np.tile(b[f].reshape(1, -1), (nenv, 1)) for f in rc.INPUT_FIELDS}
    out.update({f: np.tile(a[f].reshape(1, -1), (nenv, 1)) for f in GEO_INPUTS})
    return out


def random_geometry(pod, nenv, seed=0, pos=0.05, tilt=0.1, stiffness=0.3, spring=0.05):
    """Per-env geometry / springs around the model's own: collision geom positions + U(-pos, pos), orientations turned by up to
    `tilt` rad about a random axis (unit quaternions), spring stiffness x U(1 - stiffness, 1 + stiffness), spring references
    + U(-spring, spring) on hinge / slide joints.  [nenv][dim] arrays, collision geoms in compiled order."""
    rng = np.random.default_rng(seed)
    a = params_as_arrays(pod.params, pod)
    ng, nj, nq = pod.ngeom, pod.njnt, pod.nq
    gp = a["geom_pos"][None] + rng.uniform(-pos, pos, (nenv, ng, 3))
    ax = rng.normal(size=(nenv, ng, 3))
    ax /= np.linalg.norm(ax, axis=2, keepdims=True)
    ang = rng.uniform(0, tilt, (nenv, ng))
    dq = np.concatenate([np.cos(ang / 2)[..., None], np.sin(ang / 2)[..., None] * ax], axis=2)
    gq = np.array([[quat_mul(dq[e, g], a["geom_quat"][g]) for g in range(ng)] for e in range(nenv)])
    gq /= np.linalg.norm(gq, axis=2, keepdims=True)
    js = a["jnt_stiffness"][None] * rng.uniform(1 - stiffness, 1 + stiffness, (nenv, nj))
    qs = np.tile(a["qpos_spring"], (nenv, 1))
    for j in range(nj):
        if pod.jnt_type[j] in (2, 3):   # slide, hinge
            qs[:, pod.jnt_qposadr[j]] += rng.uniform(-spring, spring, nenv)
    return {"geom_pos": gp.reshape(nenv, -1), "geom_quat": gq.reshape(nenv, -1), "jnt_stiffness": js, "qpos_spring": qs}


def quat_mul(a, b):
    return np.array([a[0] * b[0] - a[1] * b[1] - a[2] * b[2] - a[3] * b[3], a[0] * b[1] + a[1] * b[0] + a[2] * b[3] - a[3] * b[2],
                     a[0] * b[2] - a[1] * b[3] + a[2] * b[0] + a[3] * b[1], a[0] * b[3] + a[1] * b[2] - a[2] * b[1] + a[3] * b[0]])


class HostGeomEnvModels(rc.HostEnvModels):
    """HostEnvModels that also writes the four geometry / spring inputs (where `params` has them) into the host model before it
    compiles env e's model."""

    def __init__(self, name, flags=0):
        super().__init__(name, flags)
        pod = self.m.pod
        self.nj, self.nq = pod.njnt, pod.nq
        self.v_gpos = self.m.array(P.M_GEOM_POS, 3 * self.ngeom_full)
        self.v_gquat = self.m.array(P.M_GEOM_QUAT, 4 * self.ngeom_full)
        self.v_stiff = self.m.array(P.M_JNT_STIFFNESS, self.nj)
        self.v_qspring = self.m.array(P.M_QPOS_SPRING, self.nq)

    def pod(self, params, e, set_const=True):
        if "geom_pos" in params:
            gp = np.asarray(params["geom_pos"][e]).reshape(self.ng, 3)
            for g, full in enumerate(self.fullid):
                self.v_gpos[3 * full: 3 * full + 3] = gp[g]
        if "geom_quat" in params:
            gq = np.asarray(params["geom_quat"][e]).reshape(self.ng, 4)
            for g, full in enumerate(self.fullid):
                self.v_gquat[4 * full: 4 * full + 4] = gq[g]
        if "jnt_stiffness" in params:
            self.v_stiff[:] = params["jnt_stiffness"][e]
        if "qpos_spring" in params:
            self.v_qspring[:] = params["qpos_spring"][e]
        return super().pod(params, e, set_const)


def params_as_arrays(block, pod):
    """The geometry / spring arrays of a cm_envparams_t (a CmEnvParams or the `params` member of a CmModel), trimmed."""
    nb, nv, ng, nj, nq = pod.nbody, pod.nv, pod.ngeom, pod.njnt, pod.nq
    a = lambda f, *shape: np.ctypeslib.as_array(getattr(block, f)).reshape(-1)[: int(np.prod(shape))].reshape(shape).copy()
    return {"geom_pos": a("geom_pos", ng, 3), "geom_quat": a("geom_quat", ng, 4), "jnt_stiffness": a("jnt_stiffness", nj),
            "qpos_spring": a("qpos_spring", nq), "geom_mat": a("geom_mat", ng, 9), "body_reach": a("body_reach", nb),
            "dof_stiffness": a("dof_stiffness", nv), "dof_springref": a("dof_springref", nv)}


def model_arrays(pod):
    """The same arrays from a compiled model's top-level fields (what the host compile derived)."""
    nb, nv, ng, nj, nq = pod.nbody, pod.nv, pod.ngeom, pod.njnt, pod.nq
    a = lambda f, *shape: np.ctypeslib.as_array(getattr(pod, f)).reshape(-1)[: int(np.prod(shape))].reshape(shape).copy()
    return {"geom_pos": a("geom_pos", ng, 3), "geom_quat": a("geom_quat", ng, 4), "jnt_stiffness": a("jnt_stiffness", nj),
            "qpos_spring": a("qpos_spring", nq), "geom_mat": a("geom_mat", ng, 9), "body_reach": a("body_reach", nb),
            "dof_stiffness": a("dof_stiffness", nv), "dof_springref": a("dof_springref", nv)}


def assert_geo_equal(got_block, want_pod, pod, what, fields=GEO_INPUTS + GEO_DERIVED):
    """Bit for bit against the host compile's top-level arrays of want_pod (and its own block, which must carry the same)."""
    g, w, wb = params_as_arrays(got_block, pod), model_arrays(want_pod), params_as_arrays(want_pod.params, pod)
    for f in fields:
        for ref, src in ((w, "compile"), (wb, "compiled model's own block")):
            if not np.array_equal(g[f].view(np.uint64), ref[f].view(np.uint64)):
                bad = np.argwhere(g[f] != ref[f])
                i = tuple(bad[0]) if len(bad) else ()
                raise AssertionError("%s: %s differs from the host %s at %s: %r vs %r (%d of %d entries)"
                                     % (what, f, src, i, g[f][i] if len(bad) else None, ref[f][i] if len(bad) else None, len(bad), g[f].size))


def new_blocks(pod, nenv, params):
    """rc.new_blocks, plus the geometry / spring inputs of `params` (where present) written in."""
    blocks = rc.new_blocks(pod, nenv, params)
    for e in range(nenv):
        for f in GEO_INPUTS:
            if f in params:
                dst = np.ctypeslib.as_array(getattr(blocks[e], f)).reshape(-1)
                row = np.asarray(params[f][e]).reshape(-1)
                dst[: row.size] = row
    return blocks


def garble_derived(block, fields=GEO_DERIVED):
    for f in fields:
        np.ctypeslib.as_array(getattr(block, f)).reshape(-1)[:] = -1.0


def sizeof_block():
    return ctypes.sizeof(CmEnvParams)
