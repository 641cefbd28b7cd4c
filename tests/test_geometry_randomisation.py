"""Per-env geometry and springs (CM_P_GEOM_POS / CM_P_GEOM_QUAT / CM_P_JNT_STIFFNESS / CM_P_QPOS_SPRING) on the CPU: the device's
set_const kernel deriving geom_mat / body_reach / dof_stiffness / dof_springref, and the step kernel reading them from the env's
block, executed by the wave emulator, against the host model compiler and the oracle run on each env's own compiled model.
The GPU counterpart is tests/test_geometry_randomise_gpu.py."""
import ctypes

import numpy as np
import pytest

import emu_py
import geometry_randomise_check as gc
import oracle_py
import randomise_check as rc
from cassie_amd import Model
from cassie_amd._lib import CmModel
from oracle_py import Oracle

SETCONST_ALL, SETCONST_GEOMETRY, SETCONST_SPRINGS = 1, 2, 3


def _reading_blocks(pod, geom, springs):
    """A copy of the shared model that tells the step kernel to read geometry / springs from the env's block (what
    phys_batch_randomize sets on a batch's shared model once it has randomised them)."""
    out = CmModel.from_buffer_copy(pod)
    out.env_geom, out.env_springs = geom, springs
    return out


def test_block_layout_appends_the_geometry_fields():
    assert emu_py.lib().emu_sizeof_envparams() == gc.sizeof_block() == 15824
    # the existing offsets stay where they were; the new arrays follow pair_friction
    from cassie_amd._lib import CmEnvParams
    assert CmEnvParams.pair_friction.offset + CmEnvParams.pair_friction.size == CmEnvParams.geom_pos.offset == 10192
    # the model's own block carries the compile's values
    for name in ("cassie", "cassie_hfield", "cassie_tray_box"):
        pod = Model(name).pod
        gc.assert_geo_equal(pod.params, pod, pod, name)


@pytest.mark.parametrize("name", ["cassie", "cassie_hfield", "cassie_tray_box"])
@pytest.mark.parametrize("mode", [SETCONST_ALL, SETCONST_GEOMETRY, SETCONST_SPRINGS])
def test_device_derives_geometry_and_springs_like_the_host_compile(name, mode):
    nenv = 4
    hosts = gc.HostGeomEnvModels(name)
    pod0 = Model(name).pod
    params = gc.own_params(pod0, nenv)
    if mode == SETCONST_ALL:
        params.update(rc.random_params(hosts.m, nenv, seed=7))
    params.update(gc.random_geometry(pod0, nenv, seed=17 + mode))
    blocks = gc.new_blocks(pod0, nenv, params)
    derived = {SETCONST_ALL: gc.GEO_DERIVED, SETCONST_GEOMETRY: ("geom_mat", "body_reach"),
               SETCONST_SPRINGS: ("dof_stiffness", "dof_springref")}[mode]
    for e in range(nenv):
        gc.garble_derived(blocks[e], derived)
    emu_py.set_const(pod0, blocks, nenv, mode)
    reach0 = pod0.body_reach[pod0.root_body[0]]
    moved = False
    for e in range(nenv):
        want = hosts.pod(params, e, set_const=(mode == SETCONST_ALL))
        gc.assert_geo_equal(blocks[e], want, pod0, "%s mode %d env %d" % (name, mode, e), gc.GEO_INPUTS + derived)
        if mode == SETCONST_ALL:
            rc.assert_blocks_equal(blocks[e], want.params, pod0, "%s env %d" % (name, e))
        moved |= blocks[e].body_reach[pod0.root_body[0]] != reach0
    # modes that derive only one group leave the other group's derived arrays as they were
    other = [f for f in gc.GEO_DERIVED if f not in derived]
    for e in range(nenv):
        for f in other:
            assert np.all(gc.params_as_arrays(blocks[e], pod0)[f] == gc.params_as_arrays(pod0.params, pod0)[f]), f
    if mode != SETCONST_SPRINGS:
        assert moved


def _default_rows(pod, n):
    return gc.own_params(pod, n)


def test_cassie_five_envs_300_steps_each_on_its_own_geometry_and_springs(cassie):
    """Env 0 defaults; 1 a stair box under the feet; 2 the floor tilted 5 degrees about y; 3 heel springs x 1.3 and shin spring
    references offset; 4 the pelvis sphere pushed 2.2 m out with a stair box against it that only the NEW reach lets past the
    block cull.  Every env against the oracle on its own compiled model."""
    nenv, nsteps = 5, 300
    pod0 = cassie.pod
    q0 = cassie.qpos_init()
    params = _default_rows(pod0, nenv)
    gp = params["geom_pos"].reshape(nenv, pod0.ngeom, 3)
    gq = params["geom_quat"].reshape(nenv, pod0.ngeom, 4)
    assert pod0.geom_type[0] == 0 and pod0.geom_type[1] == 6 and pod0.geom_type[16] == 2 and pod0.geom_bodyid[16] == pod0.root_body[0]
    gp[1, 1] = [0.0, 0.0, -0.96]                                   # 2 m cube, top face at z = +0.04 (tests/test_boxes.py)
    a = np.radians(5.0) / 2
    gq[2, 0] = [np.cos(a), 0.0, np.sin(a), 0.0]                   # the floor, tilted
    for j in range(pod0.njnt):
        if pod0.jnt_stiffness[j] == 1250.0:                        # heel springs
            params["jnt_stiffness"][3, j] *= 1.3
        if pod0.jnt_stiffness[j] == 1500.0:                        # knee / shin springs
            params["qpos_spring"][3, pod0.jnt_qposadr[j]] += 0.03
    gp[4, 16] = [0.0, 2.2, 0.0]                                    # the pelvis sphere, far out to the side
    rs, box = pod0.geom_rbound[16], 2
    gp[4, box] = [q0[0] + 0.02, q0[1] + 2.2 + rs + 1.0 - 0.01, q0[2] + 0.02]   # a 1 m half-size box just touching it
    params["geom_pos"] = gp.reshape(nenv, -1)
    params["geom_quat"] = gq.reshape(nenv, -1)
    hosts = gc.HostGeomEnvModels("cassie")
    pods = [hosts.pod(params, e) for e in range(nenv)]
    # the box is out of the old reach's cull bound and within the new one
    root = pod0.root_body[0]
    d = np.linalg.norm(gp[4, box] - np.array([q0[0], q0[1], q0[2]]))
    rb = pod0.geom_rbound[box] + pod0.geom_margin[box] + 0.01
    assert pod0.body_reach[root] + rb < d - 0.05 and d + 0.05 < pods[4].body_reach[root] + rb
    blocks = gc.new_blocks(pod0, nenv, params)
    emu_py.set_const(pod0, blocks, nenv, SETCONST_ALL)
    for e in range(nenv):
        gc.assert_geo_equal(blocks[e], pods[e], pod0, "env %d" % e)
    emu = emu_py.EmuBatch(_reading_blocks(pod0, 1, 1), nenv)
    emu.qpos[:] = q0
    orc = [Oracle(pods[e], q0) for e in range(nenv)]
    box_contacts = [0] * nenv
    emu.envparams = blocks
    for s in range(nsteps):
        emu.step()
        for e, o in enumerate(orc):
            o.step()
            assert (emu.info[e, 0], emu.info[e, 1]) == (o.d.ncon, o.d.nefc), (e, s)
            n = sum(1 for i in range(o.d.ncon) if box in (o.d.contact[i].geom1, o.d.contact[i].geom2) or 1 in (o.d.contact[i].geom1, o.d.contact[i].geom2))
            box_contacts[e] = max(box_contacts[e], n)
    for e in range(nenv):
        assert np.max(np.abs(emu.qpos[e] - orc[e].qpos)) < 1e-8, e
    assert not emu.warn.any()
    assert box_contacts[1] >= 2 and box_contacts[4] >= 1 and box_contacts[0] == 0
    for e in (2, 3):
        assert np.max(np.abs(emu.qpos[e] - emu.qpos[0])) > 1e-6, e


def test_hfield_terrain_geom_shifted_per_env(built):
    """cassie_hfield.xml: the terrain geom's offset differs env by env; every env against the oracle on its own model."""
    m = Model("cassie_hfield")
    pod0 = m.pod
    nenv, nsteps = 3, 200
    h = np.random.default_rng(99).random((200, 200)).astype(np.float32)
    h[95:105, 95:105] = 0
    q0 = m.qpos_init()
    q0[0] = 0.35
    params = _default_rows(pod0, nenv)
    gp = params["geom_pos"].reshape(nenv, pod0.ngeom, 3)
    hg = pod0.hfield_geom
    gp[1, hg] += [0.3, -0.2, 0.04]
    gp[2, hg] += [-0.25, 0.1, -0.03]
    params["geom_pos"] = gp.reshape(nenv, -1)
    hosts = gc.HostGeomEnvModels("cassie_hfield")
    pods = [hosts.pod(params, e) for e in range(nenv)]
    blocks = gc.new_blocks(pod0, nenv, params)
    emu_py.set_const(pod0, blocks, nenv, SETCONST_GEOMETRY)
    oracle_py.set_hfield(h)
    emu = emu_py.EmuBatch(_reading_blocks(pod0, 1, 0), nenv)
    emu.qpos[:] = q0
    emu.hfield = h.ravel().copy()
    try:
        orc = [Oracle(pods[e], q0) for e in range(nenv)]
        emu.envparams = blocks
        seen = [0] * nenv
        for s in range(nsteps):
            emu.step()
            for e, o in enumerate(orc):
                o.step()
                assert (emu.info[e, 0], emu.info[e, 1]) == (o.d.ncon, o.d.nefc), (e, s)
                seen[e] = max(seen[e], o.d.ncon)
    finally:
        oracle_py.set_hfield(None)
    assert min(seen) >= 2
    for e in range(nenv):
        assert np.max(np.abs(emu.qpos[e] - orc[e].qpos)) < 1e-8, e
    assert np.max(np.abs(emu.qpos[1] - emu.qpos[0])) > 1e-6 and np.max(np.abs(emu.qpos[2] - emu.qpos[0])) > 1e-6
