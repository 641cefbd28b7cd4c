"""The kernels that cast rays at the scene's geoms -- the range sensors, the two depth images, the height scan and the placed restart --
on the wave emulator, on the smallest cases of their own tests that still reach every branch: outputs() gives every array they
write.  tools/make_golden_scene_rays.py records them in tests/golden/scene_rays_pin.npz and tests/test_scene_rays_pin.py holds the
kernels to those bits: the geometry is shared code (csrc/scene_rays.h, ray_box of csrc/surface_kernels.h), and a change to it that
is meant to leave every kernel's answer alone can be held to that.  The emulator is built for baseline x86-64 without contraction,
so the bits do not depend on the machine.

  rays_<model>   case 1 of tests/test_rays.py on cassie and cassie_tray_box: 8 envs, 96 rays (a partial block of 64), every geom
                 kind hit, static and moving, rays at `rmin` from inside a solid
  rays_hfield    the height-field case of tests/test_rays.py: 8 envs on a bank of three terrains
  scene          case 2 of tests/test_depth_scene.py: 12 envs, 20 x 12 (partial tiles both ways), every geom in the mask
  static         case 1 of tests/test_depth.py: 12 envs of cassie_hfield, the static kernel
  scan           the stairs of tests/test_terrain.py at 16 envs: planes and boxes of any pose under 187 points
  placed         the placed restart of tests/test_placement.py on cassie's stairs, a footprint of 5 points"""
import numpy as np

import depth_scene_check as sc
import rays_cases as cs
import rays_emu_py as re_
import terrain_check as tc
import test_depth as td
import test_depth_scene as ts
import test_placement as tp
import test_rays as tr
import test_terrain as tt
from cassie_amd import Model

GOLDEN = "scene_rays_pin.npz"
PLACED_FIELDS = ("qpos", "qvel", "warn", "done")


def ray_cases():
    """-> {name: (pod, table, xpos, xquat, keywords of rays_emu_py.cast)}"""
    out = {}
    for name in ("cassie", "cassie_tray_box"):
        c = tr.definition_case(name, tr.NENV)
        out["rays_" + name] = (c["pod"], c["table"], c["xpos"], c["xquat"], dict(mask=c["every"], blocks=tt._blocks(c["pod"], c["gp"], c["gq"])))
    hf = Model("cassie_hfield")
    pod = hf.pod
    c = cs.hfield_case(hf, tr.NENV, seed=2)
    xpos, xquat = ts.emu_forward(pod, c["qpos"])
    out["rays_hfield"] = (pod, cs.foot_probe_table(pod), xpos, xquat,
                          dict(mask=sc.all_mask(pod), blocks=tt._blocks(pod, c["gp"], c["gq"]), hfield=c["bank"].reshape(-1),
                               stride=pod.hfield_nrow * pod.hfield_ncol, nterrain=len(c["bank"]), index=c["index"]))
    return out


def scene_case():
    c = ts.consistent_case(Model("cassie"), ts.NENV, seed=13)
    c["xpos"], c["xquat"] = ts.emu_forward(c["pod"], c["qpos"])
    return c


def static_case():
    return td.hfield_depth_case(Model("cassie_hfield"), 12, seed=31, nbank=4)


def scan_case():
    return tt.stairs_case(Model("cassie"), 16, seed=11)


def placed_case():
    return tp.make_case("cassie", 5)


def outputs():
    """Every case through the emulator -> {name: array}."""
    out = {}
    for name, (pod, table, xpos, xquat, kw) in ray_cases().items():
        for what, a in zip(("ranges", "ids", "normals", "warn"), re_.cast(pod, table, tr.RMIN, tr.RMAX, xpos, xquat, **kw)):
            out["%s_%s" % (name, what)] = a
    c = scene_case()
    pod = c["pod"]
    out["scene_image"], out["scene_ids"], out["scene_warn"] = ts.emu_scene(pod, c["qpos"], c["pose"][0, 3:7], sc.all_mask(pod), c["xpos"], c["xquat"],
                                                                           pose=c["pose"], blocks=tt._blocks(pod, c["gp"], c["gq"]))
    c = static_case()
    pod = c["pod"]
    out["static_image"], out["static_warn"] = td.emu_depth(pod, c["qpos"], c["cam_quat"], blocks=tt._blocks(pod, c["gp"], c["gq"]), hfield=c["bank"].reshape(-1),
                                                           stride=pod.hfield_nrow * pod.hfield_ncol, index=c["index"], nterrain=len(c["bank"]))
    c = scan_case()
    out["scan_values"], out["scan_warn"] = tt.emu_scan(c["pod"], c["qpos"], tc.grid_pattern(), blocks=tt._blocks(c["pod"], c["gp"], c["gq"]))
    got, place = tp.run_emulator(placed_case())
    for k in PLACED_FIELDS:
        out["placed_" + k] = got[k]
    out["placed_ground"] = place["ground"]
    return {k: np.ascontiguousarray(v) for k, v in out.items()}
