"""The launcher's rules for the kernels around the step kernel (csrc/small_launch.h) on the CPU, through the emulator library, in the
manner of tests/test_launch_policy.py: the grid of every launch at its edges, which of the two depth kernels an image takes, and every
refusal of a scan / depth / mask configuration with its message.  No kernel runs.  The emulator's entry points go through the same
functions (tests/emu/*.cpp), and tests/test_small_launch_gpu.py holds the launcher's last error against the same messages."""
import math

import numpy as np
import pytest

import depth_emu_py
import emu_py
from cassie_amd import Model
from cassie_amd._lib import CmModel

SCAN_SIZE = "1 .. 1024 points and a positive range"
BODY = "the body must be a child of the world whose joints are slides and at most a ball or free joint (a shared kin_simple model)"
DEPTH_SIZE = "an image of 1 .. 16384 pixels and a camera pose"
DEPTH_OPTICS = "0 < fovy < pi (radians) and 0 < near < far"
DEPTH_QUAT = "the camera's quaternion is zero"
MASK = "the mask names a geom at or above ngeom"
FOVY, NEAR, FAR = math.radians(70.0), 0.1, 6.0


def refusals(pod):
    """Every refused configuration once: (what, kind, arguments, message).  scan: (npoints, body, range); depth: (body, width, height,
    fovy, near, far, cam_quat); mask: (mask,)."""
    pelvis, unit, zero = pod.root_body[0], (1.0, 0.0, 0.0, 0.0), (0.0, 0.0, 0.0, 0.0)
    assert pod.body_parentid[pelvis] == 0 and pod.body_parentid[pelvis + 1] == pelvis and pod.ngeom < 32
    return [
        ("no points", "scan", (0, pelvis, 1.0), SCAN_SIZE),
        ("1025 points", "scan", (1025, pelvis, 1.0), SCAN_SIZE),
        ("a range of 0", "scan", (4, pelvis, 0.0), SCAN_SIZE),
        ("a scan body that is not a child of the world", "scan", (4, pelvis + 1, 1.0), BODY),
        ("no pixels", "depth", (pelvis, 0, 8, FOVY, NEAR, FAR, unit), DEPTH_SIZE),
        ("more than 16384 pixels", "depth", (pelvis, 129, 128, FOVY, NEAR, FAR, unit), DEPTH_SIZE),
        ("a fovy of 0", "depth", (pelvis, 9, 7, 0.0, NEAR, FAR, unit), DEPTH_OPTICS),
        ("a fovy of pi", "depth", (pelvis, 9, 7, math.pi, NEAR, FAR, unit), DEPTH_OPTICS),
        ("near >= far", "depth", (pelvis, 9, 7, FOVY, 2.0, 2.0, unit), DEPTH_OPTICS),
        ("a zero quaternion", "depth", (pelvis, 9, 7, FOVY, NEAR, FAR, zero), DEPTH_QUAT),
        ("a mask bit at ngeom", "mask", (1 << pod.ngeom,), MASK),
    ]


def emu_message(pod, kind, args):
    """What the shared check answers (None: accepted)."""
    if kind == "scan":
        return emu_py.scan_check(pod, *args)
    if kind == "depth":
        return emu_py.depth_check(pod, *args[:6], cam_quat=args[6])
    return emu_py.depth_geoms_check(pod, *args)


@pytest.fixture(scope="module")
def hfield_pod(built):
    return Model("cassie_hfield").pod


@pytest.mark.parametrize("which,cap", [(emu_py.EPISODES, 32), (emu_py.SCAN, 256), (emu_py.RESET, 4), (emu_py.SET_CONST, 2048),
                                       (emu_py.PARAM_SCATTER, 1024)])
def test_a_grid_is_one_workgroup_per_env_up_to_its_cap(built, which, cap):
    assert [emu_py.small_grid(which, n) for n in (1, cap - 1, cap, cap + 1, 100 * cap)] == [1, cap - 1, cap, cap, cap]


def test_the_depth_grid_is_the_job_count_up_to_2048(built):
    # 9 x 7 pixels are 2 x 1 tiles of 8 x 8: two jobs per env, the job count meets the cap at 1024 envs and passes it at 1025
    assert [emu_py.small_grid(emu_py.DEPTH, n, 9, 7) for n in (1, 1024, 1025)] == [2, 2048, 2048]
    assert [emu_py.small_grid(emu_py.DEPTH, n, 9, 7) for n in (3, 1023)] == [6, 2046]
    # one tile: an 8 x 8 image, a 1 x 1 image
    for w, h in ((8, 8), (1, 1)):
        assert [emu_py.small_grid(emu_py.DEPTH, n, w, h) for n in (1, 5, 2048, 2049)] == [1, 5, 2048, 2048]
    assert emu_py.small_grid(emu_py.DEPTH, 1, 9, 9) == 4 and emu_py.small_grid(emu_py.DEPTH, 1, 128, 128) == 256
    assert emu_py.small_grid(emu_py.DEPTH, 1 << 24, 128, 128) == 2048          # (the job count is formed in 64 bits)


def test_which_depth_kernel_an_image_takes(hfield_pod):
    pod = hfield_pod
    default, every = emu_py.depth_geoms(pod), emu_py.depth_geoms(pod, every=True)
    assert every == (1 << pod.ngeom) - 1 and default == 1 and default != every     # (geom 0 is the height field, the others move)
    assert emu_py.depth_scene_kernel(pod, default) is False
    assert emu_py.depth_scene_kernel(pod, default, ids_bound=True) is True
    assert emu_py.depth_scene_kernel(pod, every) is True and emu_py.depth_scene_kernel(pod, 0) is True
    assert emu_py.depth_scene_kernel(pod, default | 2) is True and emu_py.depth_scene_kernel(pod, default | 2, ids_bound=True) is True
    # a mask that is not the default but renders what the default renders -- it adds a moving cylinder, which neither kernel draws --
    # still goes to the scene kernel: the choice compares masks, not images
    model = CmModel.from_buffer_copy(pod)
    assert model.body_weldid[model.geom_bodyid[1]] != 0
    model.geom_type[1] = 5
    assert emu_py.depth_geoms(model) == default and emu_py.depth_scene_kernel(model, default) is False
    assert emu_py.depth_scene_kernel(model, default | 2) is True


def test_every_refusal_has_its_message(hfield_pod):
    pod = hfield_pod
    table = refusals(pod)
    assert len(table) == 11
    for what, kind, args, message in table:
        assert emu_message(pod, kind, args) == message, what
    # ... and what they refuse is the edge: the neighbours are accepted
    pelvis = pod.root_body[0]
    for npoints, scan_range in ((1, 1.0), (1024, 1.0), (4, 1e-300)):
        assert emu_py.scan_check(pod, npoints, pelvis, scan_range) is None
    for w, h, fovy, near, far in ((1, 1, FOVY, NEAR, FAR), (128, 128, FOVY, NEAR, FAR), (9, 7, 1e-6, NEAR, FAR), (9, 7, 3.14159, NEAR, FAR),
                                  (9, 7, FOVY, 2.0, 2.0000001)):
        assert emu_py.depth_check(pod, pelvis, w, h, fovy, near, far) is None
    assert emu_py.depth_check(pod, pelvis, 9, 7, FOVY, NEAR, FAR, cam_quat=(0.0, 0.0, 0.0, 1e-150)) is None
    assert emu_py.depth_geoms_check(pod, (1 << pod.ngeom) - 1) is None and emu_py.depth_geoms_check(pod, 0) is None


def test_what_else_the_shared_checks_refuse(hfield_pod):
    pod = hfield_pod
    pelvis = pod.root_body[0]
    assert emu_py.scan_check(pod, 4, pelvis, 1.0, offsets=False) == SCAN_SIZE            # no pattern
    assert emu_py.scan_check(pod, 4, pelvis, float("nan")) == SCAN_SIZE
    for body in (0, -1, pod.nbody, pod.nbody + 7):                                         # the world itself, no body at all
        assert emu_py.scan_check(pod, 4, body, 1.0) == BODY and emu_py.depth_check(pod, body, 9, 7, FOVY, NEAR, FAR) == BODY
    assert emu_py.scan_check(pod, 4, pelvis, 1.0, model_stride=1) == BODY                 # per-env models
    assert emu_py.depth_check(pod, pelvis, 9, 7, FOVY, NEAR, FAR, model_stride=1) == BODY
    assert emu_py.depth_check(pod, pelvis, 9, 7, FOVY, 0.0, FAR) == DEPTH_OPTICS and emu_py.depth_check(pod, pelvis, 9, 7, FOVY, 3.0, 2.0) == DEPTH_OPTICS
    assert emu_py.depth_check(pod, pelvis, 9, 7, FOVY, NEAR, FAR, cam_quat=(float("nan"), 0.0, 0.0, 0.0)) == DEPTH_QUAT
    assert emu_py.depth_check(pod, pelvis, 8, -1, FOVY, NEAR, FAR) == DEPTH_SIZE
    assert emu_py.depth_geoms_check(pod, 0x80000000) == MASK
    # the emulator's entry points refuse the same (they return -1; the binding asserts on it)
    qpos = np.tile(np.array(pod.qpos0[: pod.nq]), (1, 1))
    with pytest.raises(AssertionError):
        emu_py.height_scan(pod, qpos, np.zeros((4, 2)), pelvis + 1, 1.0)
    with pytest.raises(AssertionError):
        emu_py.height_scan(pod, qpos, np.zeros((4, 2)), pelvis, 0.0)
    with pytest.raises(AssertionError):
        depth_emu_py.depth_image(pod, qpos, pelvis + 1, np.zeros(3), np.array([1.0, 0, 0, 0]), 9, 7, 70.0, NEAR, FAR)
    with pytest.raises(AssertionError):
        depth_emu_py.depth_image(pod, qpos, pelvis, np.zeros(3), np.zeros(4), 9, 7, 70.0, NEAR, FAR)
