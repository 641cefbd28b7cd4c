#!/usr/bin/env python3
"""What range sensors per policy step cost config 4's loop -- 4096 cassie_hfield.xml envs, CM_DRIVE_PD_SAFE, 50 fused substeps per
launch, the batch as two env ranges on two streams, a bank of 64 terrains with a random per-env index, restarts on bench.py's
schedule (tools/depth_rate.py's loop) -- in two settings in one session, fenced timed regions:

  no_rays     the loop alone.  THE YARDSTICK.
  rays_64     the same plus a cast of 64 rays per env, range and policy step (phys_batch_rays_cast): 32 probes straight down from the
              two feet (16 along each toe) and a fan of 32 rays ahead of the pelvis in its heading frame, every geom in the mask, hit
              ids and normals bound.

--parent-lib PATH runs both legs once more, each in a child process, against another build of the library (the parent commit's): a
batch that never configures rays must run as before and the cast must not have become slower, and the yardstick for that is the parent
in the same session, not a file -- the median of this build's regions must lie within the spread of the parent's regions, leg by leg,
and the cast alone (the median of ten runs) within the parent's ten runs.

Also times the cast alone over the whole batch on an idle device and records the kernel's registers, scratch and LDS as the compiler
reports them (hipcc -Rpass-analysis=kernel-resource-usage on csrc/ray_kernel.h; null where hipcc is absent).  Prints one JSON line;
`--out` also writes it to a file.  Needs a GPU.

    python tools/ray_rate.py [--envs 4096] [--launches 20] [--warmup 10] [--repeats 10] [--only NAME] [--out profiles/ray_rate.json]
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
sys.path.insert(0, os.path.join(REPO, "tools"))

import bench  # noqa: E402
import golden_physics as G  # noqa: E402
import torch  # noqa: E402
from cassie_amd import Batch, Model  # noqa: E402
from cassie_amd import phys as P  # noqa: E402
from terrain_rate import NTERRAIN, terrain  # noqa: E402

NSUB = bench.HOLD
SETTINGS = ("no_rays", "rays_64")
KERNEL = "cassie_rays_kernel"
RMIN, RMAX = 0.01, 5.0
ALONE_RUNS = 10


def ray_table(pod):
    """32 probes straight down from the feet (16 along each toe capsule's axis) and 32 rays fanned over 120 degrees ahead of the pelvis,
    pitched down, in its heading frame."""
    toes = [g for g in range(pod.ngeom) if pod.geom_type[g] == 3 and abs(pod.geom_size[g][0] - 0.02) < 1e-9]
    rays = []
    for g in toes:
        for k in range(16):
            rays.append((pod.geom_bodyid[g], P.RAY_WORLD_DIR, [pod.geom_pos[g][0], pod.geom_pos[g][1] - 0.08 + 0.16 * k / 15, pod.geom_pos[g][2]], [0.0, 0.0, -1.0]))
    for k in range(32):
        a = np.radians(-60 + 120 * k / 31)
        rays.append((pod.root_body[0], P.RAY_HEADING, [0.1, 0.0, 0.0], [np.cos(a), np.sin(a), -0.45]))
    return rays


def kernel_resources():
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        return None
    with tempfile.TemporaryDirectory() as tmp:
        src = os.path.join(tmp, "rays.hip")
        with open(src, "w") as f:
            f.write('#include <hip/hip_runtime.h>\n#include "ray_kernel.h"\n')
        flags = ["-O3", "-std=c++17", "--offload-arch=gfx950", "-I" + os.path.join(REPO, "include"),
                 "-I" + os.path.join(REPO, "cassie-mujoco-sim_amd", "csrc"), "-ffp-contract=on", "-mllvm", "-amdgpu-sched-strategy=iterative-ilp",
                 "-mllvm", "-disable-machine-licm", "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage"]
        r = subprocess.run([hipcc] + flags + ["-c", src, "-o", os.path.join(tmp, "rays.o")], capture_output=True, text=True, timeout=600)
    at = re.search(r"Function Name: \w*%d%sE" % (len(KERNEL), KERNEL), r.stderr)
    if not at:
        return None
    text = r.stderr[at.start():]
    val = lambda key: int(re.search(key + r"[^:\n]*: *(\d+)", text).group(1))
    try:
        return {"compiled": "csrc/ray_kernel.h alone, with the Makefile's HIPFLAGS (phys_batch.hip includes the same header)",
                KERNEL: {"vgprs": val("VGPRs"), "sgprs": val("TotalSGPRs"), "scratch_bytes_per_lane": val("ScratchSize"), "lds_bytes": val("LDS Size"),
                         "waves_per_simd": val("Occupancy"), "vgpr_spills": val("VGPRs Spill"), "sgpr_spills": val("SGPRs Spill")}}
    except AttributeError:
        return None


def regions(model, n, rays, launches, warmup, repeats):
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
        ids = normals = None
        if rays:
            table = ray_table(pod)
            b.configure_rays(table, RMIN, RMAX)
            b.ray_geoms(b.depth_all_geoms())
            ids = torch.full((n, len(table)), -9, dtype=torch.int32, device="cuda")
            normals = torch.zeros((n, len(table), 3), dtype=torch.float64, device="cuda")
            b.bind_ray_ids(ids.data_ptr())
            b.bind_ray_normals(normals.data_ptr())
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
                if rays:
                    b.cast_rays(first, cnt, stream=st.cuda_stream)
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
        if rays:
            # the cast alone, over the whole batch on an idle device: HIP events round 20 launches, ten times (the median counts)
            ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            st = streams[0]
            b.cast_rays(0, n, stream=st.cuda_stream)
            torch.cuda.synchronize()
            runs = []
            for _ in range(ALONE_RUNS):
                with torch.cuda.stream(st):
                    ev0.record()
                    for _ in range(20):
                        b.cast_rays(0, n, stream=st.cuda_stream)
                    ev1.record()
                torch.cuda.synchronize()
                runs.append(1000.0 * ev0.elapsed_time(ev1) / 20)
            us = float(np.median(runs))
            v, hit = b.get(P.F_RAYS), ids.cpu().numpy()
            info.update({"cast_alone_us": us, "cast_alone_us_runs": runs, "rays_per_s_alone": n * len(table) / (us * 1e-6), "rays_per_env": len(table),
                         "value_range": [float(v.min()), float(v.max())], "fraction_of_rays_that_hit": float((hit >= 0).mean()),
                         "fraction_on_the_height_field": float((hit == pod.hfield_geom).mean()), "ray_launches": b.ray_launches()})
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
    ap.add_argument("--resources-only", action="store_true", help="the kernel's resources alone: no leg is run (needs hipcc, no GPU)")
    ap.add_argument("--parent-lib", default=None, help="another build of the library (the parent commit's): both legs, each in a child process")
    a = ap.parse_args()
    model = None if a.resources_only else Model("cassie_hfield")
    out = {"tool": "ray_rate", "model": "cassie_hfield", "envs": a.envs, "substeps_per_launch": NSUB, "launches_per_region": a.launches,
           "warmup_launches": a.warmup, "terrains_in_the_bank": NTERRAIN,
           "mode": "CM_DRIVE_PD_SAFE, 50 fused substeps per launch, two env ranges on two streams, a bank of terrains with a per-env index, "
                   "restarts on the benchmark's schedule (config 4); the cast per range behind its step launch",
           "rays": {"foot_probes": 32, "forward_fan": 32, "rmin": RMIN, "rmax": RMAX, "mask": "every geom", "ids": True, "normals": True},
           "yardstick": "no_rays", "kernel": KERNEL, "kernel_resources": kernel_resources()}
    if a.parent_lib and not a.resources_only:
        # (first, each in a process of its own: one library per process; this process has not touched the GPU yet)
        for leg in SETTINGS:
            cmd = [sys.executable, os.path.abspath(__file__), "--only", leg, "--envs", str(a.envs), "--launches", str(a.launches),
                   "--warmup", str(a.warmup), "--repeats", str(a.repeats)]
            r = subprocess.run(cmd, env=dict(os.environ, CASSIE_LIB=os.path.abspath(a.parent_lib)), capture_output=True, text=True, timeout=900)
            if r.returncode != 0:
                sys.exit("the --parent-lib leg %s failed:\n" % leg + r.stderr[-2000:])
            out["parent_" + leg] = json.loads(r.stdout.strip().splitlines()[-1])[leg]
    for name in SETTINGS:
        if a.only in (None, name) and not a.resources_only:
            out[name] = regions(model, a.envs, name != "no_rays", a.launches, a.warmup, a.repeats)
    if "no_rays" in out and "rays_64" in out:
        out["rays_64"]["cost_of_the_loop_percent"] = 100.0 * (1.0 - out["rays_64"]["env_steps_per_s_median"] / out["no_rays"]["env_steps_per_s_median"])
    for leg, key in zip(SETTINGS, ("unused_path", "rays_64")):
        if "parent_" + leg in out and leg in out:
            par, med = out["parent_" + leg], out[leg]["env_steps_per_s_median"]
            out[key + "_median_within_the_parents_regions"] = bool(par["env_steps_per_s_min"] <= med <= par["env_steps_per_s_max"])
            out[key + "_median_over_parent_median"] = med / par["env_steps_per_s_median"]
    if "parent_rays_64" in out and "rays_64" in out:
        runs, us = out["parent_rays_64"]["cast_alone_us_runs"], out["rays_64"]["cast_alone_us"]
        out["cast_alone_median_within_the_parents_runs"] = bool(min(runs) <= us <= max(runs))
        out["cast_alone_median_over_parent_median"] = us / out["parent_rays_64"]["cast_alone_us"]
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
