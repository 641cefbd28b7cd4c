"""What freeing a batch leaves behind, on the MI355X: a batch with every optional allocation switched on and torch tensors bound
in the place of four of its buffers is created, used and freed eight times over.  Every release of device memory reports a failure
through phys_last_error (csrc/device_mem.h), so a double free -- or the free of a buffer that belongs to the caller -- would change
that string across phys_batch_free; and the caller's tensors must outlive the batch with what the last launches wrote into them.
Free-memory counters are not looked at: other work shares the card."""
import ctypes

import numpy as np
import pytest

import golden_physics as G
from cassie_amd import Batch, Model
from cassie_amd import phys as P
from cassie_amd._lib import CmModel, lib
from derive_check import foot_ids

pytestmark = pytest.mark.gpu

N, CYCLES = 256, 8
LEFT, RIGHT = 3, 5          # columns beside the field in the wider tensors of the strided bindings
SCAN_RANGE = 2.0            # (the pelvis starts 1 m above the ground)
FILL = -3.25                # what those columns, and every tensor no launch may touch, must still hold at the end


def free_checked(b):
    """phys_batch_free must leave phys_last_error as it found it: no release failed."""
    before = lib().phys_last_error()
    b.close()
    assert lib().phys_last_error() == before, (before, lib().phys_last_error())


def terrains(pod, count):
    out = []
    for k in range(count):
        h = np.random.default_rng(70 + k).random((pod.hfield_nrow, pod.hfield_ncol)).astype(np.float32) * np.float32(0.1 * (k + 1))
        h[95:105, 95:105] = 0
        out.append(h)
    return np.stack(out)


def pattern(points):
    return np.stack([np.linspace(-0.5, 0.5, points), np.linspace(0.3, -0.3, points)], axis=1)


def one_cycle(model, cycle):
    import torch
    pod, h = model.pod, ctypes.c_void_p
    rng = np.random.default_rng(100 + cycle)
    q0 = np.tile(model.qpos_init(), (N, 1))
    for e in range(N):
        q0[e, 0], q0[e, 1] = G.start_xy("cassie_hfield", e)
    bank = terrains(pod, 3)
    points = (12, 20)

    def wide(dim):
        return torch.full((N, LEFT + dim + RIGHT), FILL, dtype=torch.float64, device="cuda")

    def ints():
        return torch.full((N,), 77, dtype=torch.int32, device="cuda")

    # two tensors per binding (bind, then bind again), a third for the scan once it has been configured again
    qpos_t, done_t, index_t = [wide(pod.nq), wide(pod.nq)], [ints(), ints()], [ints(), ints()]
    scan_t = [wide(points[0]), wide(points[0]), wide(points[1])]
    for t in index_t:
        t.zero_()
    torch.cuda.synchronize()

    b = Batch(model, N)
    # ---- every optional allocation
    assert lib().phys_batch_forward_kinematics(h(b._h), None) == 0        # (before the drive mode: the pass refuses one)
    b.set_drive_mode(P.DRIVE_TORQUE)
    assert lib().phys_batch_enable_ext(h(b._h), 1) == 0
    b.derive(foot_ids(model))
    b.randomize(P.P_DOF_DAMPING, np.tile(np.array(pod.dof_damping[: pod.nv]), (N, 1)) * rng.uniform(0.9, 1.1, (N, 1)))
    b.enable_episodes(min_height=0.4, max_steps=1)
    b.set_reset_bank(b.make_reset_bank(q0[:4]))
    b.set_hfield_bank(bank)
    assert b.terrain_index
    b.configure_scan(pattern(points[0]), pod.root_body[0], SCAN_RANGE)
    # ---- bind, and bind again
    for k in range(2):
        b.bind(P.F_QPOS, qpos_t[k].data_ptr() + 8 * LEFT, row_stride=LEFT + pod.nq + RIGHT)
        b.bind_episode(P.EP_DONE, done_t[k].data_ptr())
        b.bind_terrain_index(index_t[k].data_ptr())
        b.bind(P.F_HEIGHT_SCAN, scan_t[k].data_ptr() + 8 * LEFT, row_stride=LEFT + points[0] + RIGHT)
    # ---- another pattern: the batch drops the caller's tensor for a buffer of its own of the new size, until the caller binds again
    b.configure_scan(pattern(points[1]), pod.root_body[0], SCAN_RANGE)
    assert b.device_ptr(P.F_HEIGHT_SCAN) != scan_t[1].data_ptr() + 8 * LEFT and b.dim(P.F_HEIGHT_SCAN) == points[1]
    b.bind(P.F_HEIGHT_SCAN, scan_t[2].data_ptr() + 8 * LEFT, row_stride=LEFT + points[1] + RIGHT)
    # ---- one step, and the launches that write the other three tensors
    ids = rng.integers(0, 3, N).astype(np.int32)
    b.set(P.F_QPOS, q0)
    b.set_terrain(ids)
    b.step(10)
    b.height_scan()
    b.end_episodes(restart=True)
    want = dict(qpos=b.get(P.F_QPOS), scan=b.get(P.F_HEIGHT_SCAN), done=b.episodes()[0])
    free_checked(b)

    # ---- the caller's tensors outlive the batch, with what the last launches wrote
    torch.cuda.synchronize()
    got = [t.cpu().numpy() for t in (qpos_t[1], scan_t[2], done_t[1], index_t[1])]
    for a, key, dim in ((got[0], "qpos", pod.nq), (got[1], "scan", points[1])):
        assert np.array_equal(a[:, LEFT:LEFT + dim], want[key]), key
        assert np.all(a[:, :LEFT] == FILL) and np.all(a[:, LEFT + dim:] == FILL), key
    assert np.isfinite(want["qpos"]).all() and not np.array_equal(want["qpos"], q0)
    assert (np.abs(want["scan"]) < SCAN_RANGE).any()                              # the scan met the terrain
    assert np.array_equal(got[2], want["done"]) and want["done"].all()     # (max_steps = 1: every episode ended)
    assert np.array_equal(got[3], ids)
    # ... and the ones it was bound to before saw no launch and were not freed under the caller either
    for t in (qpos_t[0], scan_t[0], scan_t[1]):
        assert bool((t == FILL).all())
    assert bool((done_t[0] == 77).all()) and bool((index_t[0] == 0).all())


def per_env_models(model):
    """Per-env models (they exclude the parameter blocks and the scan of the batch above): expanded, back to one, expanded again."""
    pod = model.pod
    b = Batch(model, N)
    b.set_hfield(G.terrain("cassie_hfield"))
    b.set_hfield(np.zeros(pod.hfield_nrow * pod.hfield_ncol, dtype=np.float32), env=3)   # (one grid per env)
    heavy = CmModel.from_buffer_copy(pod)
    heavy.body_mass[pod.root_body[0]] *= 2          # (the pelvis; body 1 of this model is the terrain)
    b.set_model(heavy, env=1)
    b.set_model(pod, -1)
    b.set_model(heavy, env=1)
    b.set(P.F_QPOS, np.tile(model.qpos_init(), (N, 1)))
    b.step(10)
    q = b.get(P.F_QPOS)
    assert np.array_equal(q[0], q[2]) and not np.array_equal(q[0], q[1])
    free_checked(b)


def test_create_use_and_free_eight_times_leaves_no_error_and_the_callers_tensors_alone(built):
    model = Model("cassie_hfield")
    for cycle in range(CYCLES):
        one_cycle(model, cycle)
        per_env_models(model)
