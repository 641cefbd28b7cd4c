#!/usr/bin/env python3
"""What a depth image per policy step costs config 4's loop -- 4096 cassie_hfield.xml envs, CM_DRIVE_PD_SAFE, 50 fused substeps per
launch, the batch as two env ranges on two streams, a bank of 64 terrains with a random per-env index, restarts on bench.py's
schedule (tools/terrain_rate.py's `bank` leg) -- in four settings in one session, fenced timed regions:

  no_depth               the loop alone.  THE YARDSTICK (the step kernels are those of tools/terrain_rate.py's bank leg).
  depth_64x48            the same plus a 64 x 48 depth image per range and policy step (phys_batch_depth_image): the default geoms,
                         the static kernel.
  depth_64x48_all_geoms  ... with every geom in the mask (Batch.depth_geoms(moving=True)): the scene kernel, the robot's own sphere
                         and capsules drawn where the step launch in front of it left the bodies.
  depth_128x128          the default geoms, 128 x 128.

--parent-lib PATH runs the depth_64x48 and depth_64x48_all_geoms legs once more, each in a child process, against another build of the
library (the parent commit's): neither kernel must have become slower, and the yardstick for that is the parent in the same session,
not a file -- this build's median within the parent's ten regions, and its launch alone (the median of ten runs) within the parent's
ten runs.

The camera is the reference's `egocentric` one in spirit: on the pelvis, pitched 45 degrees down, fovy 65.5, near 0.01, far 5.  Also
times the depth launch alone over the whole batch on an idle device, for every leg, and records both kernels' registers, scratch and
LDS as the compiler reports them (hipcc -Rpass-analysis=kernel-resource-usage on csrc/depth_kernel.h; null where hipcc is absent).
Prints one JSON line; `--out` also writes it to a file.  Needs a GPU.

    python tools/depth_rate.py [--envs 4096] [--launches 20] [--warmup 10] [--repeats 10] [--only NAME] [--out profiles/depth_rate.json]
                               [--resources-only] [--parent-lib PATH]
"""
import argparse
import json
import os
import re
import shutil
import subprocess
import sys
import tempfile
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "cassie-mujoco-sim_amd"))
sys.path.insert(0, os.path.join(REPO, "tests"))
sys.path.insert(0, REPO)

import bench  # noqa: E402
import golden_physics as G  # noqa: E402
import torch  # noqa: E402
from cassie_amd import Batch, Model  # noqa: E402
from cassie_amd import phys as P  # noqa: E402
from terrain_rate import NTERRAIN, terrain  # noqa: E402

NSUB = bench.HOLD
SETTINGS = {"no_depth": None, "depth_64x48": (64, 48), "depth_64x48_all_geoms": (64, 48), "depth_128x128": (128, 128)}
ALL_GEOMS = {"depth_64x48_all_geoms"}
PARENT_LEGS = ("depth_64x48", "depth_64x48_all_geoms")     # what --parent-lib runs once more
ALONE_RUNS = 10
KERNELS = ("cassie_depth_kernel", "cassie_depth_scene_kernel")
CAM_POS, FOVY, NEAR, FAR, PITCH = (0.1, 0.0, 0.25), 65.5, 0.01, 5.0, 45.0


def camera_quat(pitch_deg):
    """Looking along the body's +x, pitched down (the camera looks along -z of its frame, +x right, +y up)."""
    a = np.radians(pitch_deg) / 2
    w1, x1, y1, z1 = 0.5, 0.5, -0.5, -0.5
    w2, x2, y2, z2 = np.cos(a), -np.sin(a), 0.0, 0.0
    return np.array([w1 * w2 - x1 * x2 - y1 * y2 - z1 * z2, w1 * x2 + x1 * w2 + y1 * z2 - z1 * y2,
                     w1 * y2 - x1 * z2 + y1 * w2 + z1 * x2, w1 * z2 + x1 * y2 - y1 * x2 + z1 * w2])


def kernel_resources():
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        return None
    with tempfile.TemporaryDirectory() as tmp:
        src = os.path.join(tmp, "depth.hip")
        with open(src, "w") as f:
            f.write('#include <hip/hip_runtime.h>\n#include "depth_kernel.h"\n')
        flags = ["-O3", "-std=c++17", "--offload-arch=gfx950", "-I" + os.path.join(REPO, "include"),
                 "-I" + os.path.join(REPO, "cassie-mujoco-sim_amd", "csrc"), "-ffp-contract=on", "-mllvm", "-amdgpu-sched-strategy=iterative-ilp",
                 "-mllvm", "-disable-machine-licm", "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage"]
        r = subprocess.run([hipcc] + flags + ["-c", src, "-o", os.path.join(tmp, "depth.o")], capture_output=True, text=True, timeout=600)
    out = {"compiled": "csrc/depth_kernel.h alone, with the Makefile's HIPFLAGS (phys_batch.hip includes the same header)"}
    for kernel in KERNELS:
        at = re.search(r"Function Name: \w*%d%sE" % (len(kernel), kernel), r.stderr)
        if not at:
            return None
        text = r.stderr[at.start():]
        val = lambda key: int(re.search(key + r"[^:\n]*: *(\d+)", text).group(1))
        try:
            out[kernel] = {"vgprs": val("VGPRs"), "sgprs": val("TotalSGPRs"), "scratch_bytes_per_lane": val("ScratchSize"), "lds_bytes": val("LDS Size"),
                           "waves_per_simd": val("Occupancy"), "vgpr_spills": val("VGPRs Spill"), "sgpr_spills": val("SGPRs Spill")}
        except AttributeError:
            return None
    return out


def regions(model, n, size, launches, warmup, repeats, all_geoms=False):
    pod = model.pod
    b = Batch(model, n)
    try:
        rng = np.random.default_rng(3)
        b.set_hfield_bank(np.stack([terrain(99 + k) for k in range(NTERRAIN)]))
        b.set_terrain(rng.integers(0, NTERRAIN, n).astype(np.int32))
        q0 = np.tile(model.qpos_init(), (n, 1))
        for e in range(n):
            q0[e, 0], q0[e, 1] = G.start_xy("cassie_hfield", e)
        b.set(P.F_QPOS, q0)
        b.forward()
        sens0 = b.get(P.F_SENSORDATA, 0, 1)[0]
        b.set(P.F_PD_KP, np.tile(bench.PD_KP, (n, 1)))
        b.set(P.F_PD_KD, np.tile(bench.PD_KD, (n, 1)))
        b.set(P.F_PD_PTARGET, bench.PD_OFFSET + np.random.default_rng(1).uniform(-0.3, 0.3, (n, 10)))
        b.set_drive_mode(P.DRIVE_PD_SAFE)
        init_row = torch.from_numpy(np.concatenate([model.qpos_init(), sens0])).cuda()
        if size:
            b.configure_depth(pod.root_body[0], CAM_POS, camera_quat(PITCH), size[0], size[1], FOVY, NEAR, FAR)
            if all_geoms:
                b.depth_geoms(moving=True)
        b.sync()
        torch.cuda.synchronize()
        streams, half = [torch.cuda.Stream(), torch.cuda.Stream()], n // 2
        ranges = [(0, half), (half, n - half)]
        policy_step = [0]

        def launch():
            p = policy_step[0]
            policy_step[0] += 1
            for (first, cnt), st in zip(ranges, streams):
                r0, k = bench.rows_of_group_in_range(bench.restart_group(p), 0, first, cnt)
                if k:
                    b.reset_envs(r0, bench.NGROUP, k, init_row.data_ptr(), init_row.data_ptr() + 8 * pod.nq, st.cuda_stream)
                b.step_range(first, cnt, NSUB, st.cuda_stream)
                if size:
                    b.depth_image(first, cnt, stream=st.cuda_stream)
        for _ in range(warmup):
            launch()
        out = []
        for _ in range(repeats):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(launches):
                launch()
            torch.cuda.synchronize()
            out.append(n * NSUB * launches / (time.perf_counter() - t0))
        info = {"env_steps_per_s_median": float(np.median(out)), "env_steps_per_s_min": float(min(out)), "env_steps_per_s_max": float(max(out)),
                "regions": out, "envs_with_warnings": int(b.warnings()[0].astype(bool).sum())}
        if size:
            # the depth launch alone, over the whole batch on an idle device: HIP events round 20 launches, ten times (the median counts)
            ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            st = streams[0]
            b.depth_image(0, n, stream=st.cuda_stream)
            torch.cuda.synchronize()
            runs = []
            for _ in range(ALONE_RUNS):
                with torch.cuda.stream(st):
                    ev0.record()
                    for _ in range(20):
                        b.depth_image(0, n, stream=st.cuda_stream)
                    ev1.record()
                torch.cuda.synchronize()
                runs.append(1000.0 * ev0.elapsed_time(ev1) / 20)
            us = float(np.median(runs))
            info["depth_launch_alone_us"] = us
            info["depth_launch_alone_us_runs"] = runs
            info["rays_per_s_alone"] = n * size[0] * size[1] / (us * 1e-6)
            v = b.get(P.F_DEPTH)
            info["image"] = [size[0], size[1]]
            info["depth_value_range"] = [float(v.min()), float(v.max())]
            info["fraction_of_rays_that_hit"] = float((v < FAR).mean())
            try:
                info["launches_static_kernel_scene_kernel"] = list(b.depth_launches())
            except AttributeError:          # (--parent-lib: a build of the library from before the scene kernel)
                pass
        return info
    finally:
        b.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--only", choices=list(SETTINGS), default=None, help="one setting only (e.g. under a kernel trace)")
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    ap.add_argument("--resources-only", action="store_true", help="the kernels' resources alone: no leg is run (needs hipcc, no GPU)")
    ap.add_argument("--parent-lib", default=None, help="another build of the library (the parent commit's): its two 64 x 48 legs, each in a child process")
    a = ap.parse_args()
    model = None if a.resources_only else Model("cassie_hfield")
    out = {"tool": "depth_rate", "model": "cassie_hfield", "envs": a.envs, "substeps_per_launch": NSUB, "launches_per_region": a.launches,
           "warmup_launches": a.warmup, "terrains_in_the_bank": NTERRAIN,
           "mode": "CM_DRIVE_PD_SAFE, 50 fused substeps per launch, two env ranges on two streams, a bank of terrains with a per-env index, "
                   "restarts on the benchmark's schedule (config 4); the depth image per range behind its step launch",
           "camera": {"body": "pelvis", "pos": list(CAM_POS), "pitch_down_deg": PITCH, "fovy_deg": FOVY, "near": NEAR, "far": FAR},
           "yardstick": "no_depth", "kernels": list(KERNELS), "kernel_resources": kernel_resources()}
    if a.parent_lib and not a.resources_only:
        # (first, each in a process of its own: one library per process; this process has not touched the GPU yet)
        for leg in PARENT_LEGS:
            cmd = [sys.executable, os.path.abspath(__file__), "--only", leg, "--envs", str(a.envs), "--launches", str(a.launches),
                   "--warmup", str(a.warmup), "--repeats", str(a.repeats)]
            r = subprocess.run(cmd, env=dict(os.environ, CASSIE_LIB=os.path.abspath(a.parent_lib)), capture_output=True, text=True, timeout=900)
            if r.returncode != 0:
                sys.exit("the --parent-lib leg %s failed:\n" % leg + r.stderr[-2000:])
            out["parent_" + leg] = json.loads(r.stdout.strip().splitlines()[-1])[leg]
    for name, size in SETTINGS.items():
        if a.only in (None, name) and not a.resources_only:
            out[name] = regions(model, a.envs, size, a.launches, a.warmup, a.repeats, all_geoms=name in ALL_GEOMS)
    if "no_depth" in out:
        base = out["no_depth"]["env_steps_per_s_median"]
        for name in SETTINGS:
            if name != "no_depth" and name in out:
                out[name]["cost_of_the_loop_percent"] = 100.0 * (1.0 - out[name]["env_steps_per_s_median"] / base)
    for leg, key in zip(PARENT_LEGS, ("static_leg", "all_geoms_leg")):
        if "parent_" + leg in out and leg in out:
            par, this = out["parent_" + leg], out[leg]
            med = this["env_steps_per_s_median"]
            out[key + "_median_within_the_parents_regions"] = bool(par["env_steps_per_s_min"] <= med <= par["env_steps_per_s_max"])
            out[key + "_median_over_parent_median"] = med / par["env_steps_per_s_median"]
            runs, us = par["depth_launch_alone_us_runs"], this["depth_launch_alone_us"]
            out[key + "_launch_alone_median_within_the_parents_runs"] = bool(min(runs) <= us <= max(runs))
            out[key + "_launch_alone_median_over_parent_median"] = us / par["depth_launch_alone_us"]
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
