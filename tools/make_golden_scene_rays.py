"""Generates tests/golden/scene_rays_pin.npz: what the wave emulator makes of the cases of tests/scene_rays_pin.py -- ranges or images,
ids, normals and warning words of the kernels that cast rays at the scene's geoms (range sensors, depth images, height scan, placed
restart).  tests/test_scene_rays_pin.py requires these bits.  Run it at the commit whose answers are to be kept (make emu first), BEFORE
a change to the shared geometry (csrc/scene_rays.h, csrc/surface_kernels.h) that is meant to leave them alone; a change that is meant
to move them says so and records the file anew."""
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "cassie-mujoco-sim_amd"))
sys.path.insert(0, os.path.join(REPO, "tests"))
import scene_rays_pin as pin  # noqa: E402

out = pin.outputs()
path = os.path.join(REPO, "tests", "golden", pin.GOLDEN)
np.savez_compressed(path, **out)
print("wrote", path, os.path.getsize(path), "bytes;", {k: v.shape for k, v in out.items()})
