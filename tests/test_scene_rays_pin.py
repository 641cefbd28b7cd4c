"""The kernels that cast rays at the scene's geoms, bit for bit what they were: the emulator's outputs on the cases of
tests/scene_rays_pin.py against tests/golden/scene_rays_pin.npz (tools/make_golden_scene_rays.py).  The tests of the kernels' own
files hold them to their definitions within a tolerance; this one holds shared geometry code (csrc/scene_rays.h, ray_box of
csrc/surface_kernels.h) to the exact answers of the separate copies it replaced, and every later edit of it to the same."""
import os

import numpy as np

import scene_rays_pin as pin


def test_every_output_equals_the_recorded_bits(built):
    want = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", pin.GOLDEN))
    got = pin.outputs()
    assert sorted(got) == sorted(want.files)
    for k in sorted(got):
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, k
        assert np.array_equal(got[k], want[k]), "%s: %d of %d entries differ" % (k, int((got[k] != want[k]).sum()), got[k].size)
    # the cases reach what they are there for: hits and misses, rays from inside a solid, ids of moving geoms, restarts put down
    assert (got["rays_cassie_ids"] >= 0).any() and (got["rays_cassie_ids"] < 0).any() and np.abs(got["rays_cassie_tray_box_normals"]).max() > 0.5
    assert len(np.unique(got["scene_ids"])) > 6 and got["placed_done"].sum() >= 20
