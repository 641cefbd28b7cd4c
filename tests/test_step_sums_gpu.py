"""The step-sums block on the device (include/cassie_phys.h: phys_batch_step_sums_enable; csrc/cm_model.h: CM_SUM_*).

THE REFERENCE IS THE EXISTING ONE-SUBSTEP PATH, not the new code: a twin batch with the sums off and the read-out block on is stepped
nsub times, one substep per launch; after every launch ctrl (clipped to ctrlrange), actuator_velocity, PHYS_F_BODY_CFRC and the contact
list's bodies are read and summed in numpy in substep order (sums_emu_py.Reference).  Against it the accumulating launch's COUNT,
BODY_CFRC, BODY_TOUCH and the four actuator sums must be equal BIT FOR BIT, BODY_CFRC_MAX2 to 1e-14 relative, and its final qpos / qvel
bitwise the twin's."""
import ctypes

import numpy as np
import pytest

import bench
import golden_physics as G
import sums_emu_py as S
from cassie_amd import Batch, Model
from cassie_amd import phys as P
from cassie_amd._lib import lib

pytestmark = pytest.mark.gpu


def _batch(model, n, mode, seed=5):
    """n envs of model a few millimetres about the floor's contact margin and falling (feet make contact in the middle of a launch),
    joints and velocities scattered; CM_DRIVE_PD_SAFE with scattered targets, or CM_DRIVE_OFF with constant ctrl, some of it past ctrlrange."""
    rng = np.random.default_rng(seed)
    pod = model.pod
    q = np.tile(model.qpos_init(), (n, 1))
    q[:, 2] += rng.uniform(-0.006, 0.001, n)
    q[:, 7:] += rng.uniform(-0.01, 0.01, (n, pod.nq - 7))
    v = rng.uniform(-0.05, 0.05, (n, pod.nv))
    v[:, 2] = -1.0
    hf = G.terrain(model.name)
    if hf is not None:
        for e in range(n):
            q[e, 0], q[e, 1] = G.start_xy(model.name, e)
    b = Batch(model, n)
    if hf is not None:
        b.set_hfield(hf)
    b.set(P.F_QPOS, q)
    b.set(P.F_QVEL, v)
    if mode == P.DRIVE_OFF:
        hi = np.array([pod.act_ctrlrange[u][1] for u in range(pod.nu)])
        b.set(P.F_CTRL, hi * rng.uniform(-1.3, 1.3, (n, pod.nu)))
    else:
        b.forward()
        b.set(P.F_PD_KP, np.tile(bench.PD_KP, (n, 1)))
        b.set(P.F_PD_KD, np.tile(bench.PD_KD, (n, 1)))
        b.set(P.F_PD_PTARGET, bench.PD_OFFSET + rng.uniform(-0.4, 0.4, (n, 10)))
        b.set_drive_mode(mode)
    b.sync()
    return b


def _reference(model, n, mode, nsub, seed=5):
    """The twin: sums off, read-out block on, one substep per launch -> (Reference, the twin's final qpos, qvel)."""
    L, h = lib(), ctypes.c_void_p
    twin = _batch(model, n, mode, seed)
    try:
        assert L.phys_batch_enable_ext(h(twin._h), 1) == 0
        ext = (S.CmExt * n)()
        ref = S.Reference(model.pod, n)
        for _ in range(nsub):
            twin.step(1)
            assert L.phys_batch_download_ext(h(twin._h), ext, 0, n) == 0
            ref.add(twin.get(P.F_CTRL), twin.get(P.F_ACTUATOR_VELOCITY), twin.get(P.F_BODY_CFRC), S.ext_contacts(ext, n))
        w, _ = twin.warnings()
        assert not (w & P.WARN_DIVERGED).any()
        return ref, twin.get(P.F_QPOS), twin.get(P.F_QVEL)
    finally:
        twin.close()


@pytest.mark.parametrize("name, mode", [("cassie", P.DRIVE_PD_SAFE), ("cassie_hfield", P.DRIVE_OFF), ("cassie_tray_box", P.DRIVE_OFF)])
def test_a_fused_launch_sums_what_single_substeps_leave(name, mode, built):
    model = Model(name)
    n, nsub = 64, 12
    ref, q, v = _reference(model, n, mode, nsub)
    feet = [model.name2id(1, "left-foot"), model.name2id(1, "right-foot")]
    touch = S.views(model.pod, ref.raw)["body_touch"][:, feet]
    print(name, "foot touches:", np.unique(touch, return_counts=True))
    assert touch.max() > 0, "no foot touched the ground"
    if name == "cassie":
        assert ((touch > 0) & (touch < nsub)).any(), "no foot made contact in the middle of the launch"
    # the launcher's forms: the two-wave fast kernel's FEAT_SUMS sibling (+ passes), one wave per env (the full form alone), fast rows off
    for label, tune in (("two-wave fast", lambda b: None), ("one wave per env", lambda b: b.set_waves_per_env(1)), ("fast rows off", lambda b: b.set_fast_rows(False))):
        b = _batch(model, n, mode)
        try:
            tune(b)
            b.enable_step_sums()
            b.step(nsub)
            got = b.step_sums()
            S.compare(model.pod, got["raw"], ref.raw, (name, label))
            assert (got["count"] == nsub).all()
            assert b.get(P.F_QPOS).tobytes() == q.tobytes() and b.get(P.F_QVEL).tobytes() == v.tobytes(), (name, label)
            # a launch zeroes before it adds: the same launch again does not stack on the first
            b.step(nsub)
            assert (b.step_sums()["count"] == nsub).all()
            # forward passes and derive() leave the block alone
            before = b.get(P.F_STEP_SUMS).tobytes()
            b.forward()
            assert b.get(P.F_STEP_SUMS).tobytes() == before
        finally:
            b.close()


def test_the_chunks_of_a_launch_add_in_substep_order(cassie):
    """2048 envs x 10 substeps (CHUNK_MIN_ENVS, 2 x CHUNK_MIN_SUBSTEPS): the smallest launch that goes in chunks."""
    n, nsub = 2048, 10
    ref, q, v = _reference(cassie, n, P.DRIVE_PD_SAFE, nsub, seed=6)
    b = _batch(cassie, n, P.DRIVE_PD_SAFE, seed=6)
    try:
        b.set_chunks(2)
        b.enable_step_sums()
        b.step_range(0, n, nsub)
        got = b.step_sums()
        w, _ = b.warnings()
        assert not (w & (P.WARN_DIVERGED | P.WARN_CHUNK_PLACEMENT)).any()
        S.compare(cassie.pod, got["raw"], ref.raw, "two chunks")
        assert (got["count"] == nsub).all()
        assert b.get(P.F_QPOS).tobytes() == q.tobytes() and b.get(P.F_QVEL).tobytes() == v.tobytes()
    finally:
        b.close()


def test_ranges_on_two_streams_own_their_rows(cassie):
    import torch
    n, half, nsub = 128, 64, 12
    ref, _, _ = _reference(cassie, n, P.DRIVE_PD_SAFE, nsub, seed=7)
    ref_short, _, _ = _reference(cassie, n, P.DRIVE_PD_SAFE, 5, seed=7)
    b = _batch(cassie, n, P.DRIVE_PD_SAFE, seed=7)
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    try:
        b.enable_step_sums()
        # a launch over the first range: the second range's rows stay what they were (the block's first contents: zero)
        b.step_range(0, half, 5, streams[0].cuda_stream)
        streams[0].synchronize()
        got = b.get(P.F_STEP_SUMS)
        S.compare(cassie.pod, got[:half], ref_short.raw[:half], "first range, 5 substeps")
        assert not got[half:].any()
        b.close()
        # two ranges, each zeroed and summed by its own launch on its own stream
        b = _batch(cassie, n, P.DRIVE_PD_SAFE, seed=7)
        b.enable_step_sums()
        for k, st in enumerate(streams):
            b.step_range(k * half, half, nsub, st.cuda_stream)
        for st in streams:
            st.synchronize()
        got = b.get(P.F_STEP_SUMS)
        S.compare(cassie.pod, got, ref.raw, "two ranges")
        # ... and a later launch over the second range alone leaves the first range's rows alone
        first = got[:half].tobytes()
        b.step_range(half, half, 3, streams[1].cuda_stream)
        streams[1].synchronize()
        got = b.get(P.F_STEP_SUMS)
        assert got[:half].tobytes() == first and (got[half:, P.SUM_COUNT] == 3).all()
    finally:
        b.close()


def test_a_bound_tensor_receives_the_block_and_off_means_todays_launches(cassie):
    import torch
    n, nsub = 1024, 6       # (more than SMALL_BATCH envs: a launch of any length takes the fast kernel)
    ref, _, _ = _reference(cassie, n, P.DRIVE_OFF, nsub, seed=8)
    b = _batch(cassie, n, P.DRIVE_OFF, seed=8)
    try:
        b.set_inplace(0)
        t = torch.full((n, P.SUM_DIM), float("nan"), dtype=torch.float64, device="cuda")
        b.bind(P.F_STEP_SUMS, t.data_ptr())
        b.step(1)
        assert b.form_launches() == (1, 0)                 # off: a lean fast kernel, and the tensor is nobody's
        b.sync()
        assert torch.isnan(t).all()
        b.enable_step_sums()
        b.step(nsub)
        b.sync()
        torch.cuda.synchronize()
        assert b.form_launches() == (1, 0)                 # (the accumulating launch took the FEAT_SUMS sibling: not a launch of the lean forms)
        got = t.cpu().numpy()
        assert (got[:, P.SUM_COUNT] == nsub).all() and np.abs(got[:, P.SUM_ACT_FORCE: P.SUM_ACT_FORCE + 10]).min() > 0
        # (the twin started from the same state one substep earlier: compare a launch from the same state instead)
        c = _batch(cassie, n, P.DRIVE_OFF, seed=8)
        try:
            c.enable_step_sums()
            c.bind(P.F_STEP_SUMS, t.data_ptr())
            c.step(nsub)
            c.sync()
            S.compare(cassie.pod, t.cpu().numpy(), ref.raw, "bound tensor")
        finally:
            c.close()
        b.enable_step_sums(False)
        t.fill_(float("nan"))
        torch.cuda.synchronize()
        b.step(nsub)
        b.sync()
        assert b.form_launches() == (2, 0)                 # off again: the lean form's launches are counted again ...
        assert torch.isnan(t).all()                        # ... and nothing touches the block
    finally:
        b.close()
