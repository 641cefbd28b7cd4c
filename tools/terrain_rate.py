#!/usr/bin/env python3
"""What per-env terrains and the height scan cost config 4's loop -- 4096 cassie_hfield.xml envs, CM_DRIVE_PD_SAFE, 50 fused substeps
per launch, the batch as two env ranges on two streams, restarts on bench.py's schedule -- in four settings, fenced timed regions:

  shared       one grid shared by all envs (phys_batch_set_hfield).  THE YARDSTICK; `--parent-lib` runs this leg again, in a child
               process, on another build of the library (the parent commit's: CASSIE_LIB), in the same session.
  per_env      one grid per env through phys_batch_set_hfield_env (655 MB at 4096 envs).
  bank         a bank of 64 terrains and a random per-env index (phys_batch_set_hfield_bank).
  bank_scan    the same plus a 187-point height scan per range per policy step (phys_batch_height_scan).

All terrains are the rough terrain of the benchmark (random elevations, flat start patch) with different seeds.  Prints one JSON line:
the regions of each setting (env-steps per second), the device memory the batch and its terrains hold, and the scan launch's own time
on an idle device.  Needs a GPU.

    python tools/terrain_rate.py [--envs 4096] [--launches 20] [--warmup 10] [--repeats 10] [--only NAME] [--parent-lib PATH]
"""
import argparse
import json
import os
import subprocess
import sys
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

NSUB = bench.HOLD
SETTINGS = ("shared", "per_env", "bank", "bank_scan")
NTERRAIN, SCAN_POINTS = 64, (17, 11)


def terrain(seed):
    h = np.random.default_rng(seed).random((200, 200)).astype(np.float32)
    h[95:105, 95:105] = 0
    return h


def regions(model, n, setting, launches, warmup, repeats):
    pod = model.pod
    torch.cuda.synchronize()
    free0 = torch.cuda.mem_get_info()[0]
    b = Batch(model, n)
    try:
        rng = np.random.default_rng(3)
        if setting == "shared":
            b.set_hfield(terrain(99))
        elif setting == "per_env":
            for e in range(n):
                b.set_hfield(terrain(99 + e % NTERRAIN), env=e)
        else:
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
        scan = setting == "bank_scan"
        if scan:
            nx, ny = SCAN_POINTS
            xs, ys = (np.arange(nx) - (nx - 1) / 2) * 0.1 + 0.3, (np.arange(ny) - (ny - 1) / 2) * 0.1
            b.configure_scan(np.array([[x, y] for x in xs for y in ys]), pod.root_body[0], 1.0)
        b.sync()
        torch.cuda.synchronize()
        held = free0 - torch.cuda.mem_get_info()[0]
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
                if scan:
                    b.height_scan(first, cnt, stream=st.cuda_stream)
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
                "regions": out, "envs_with_warnings": int(b.warnings()[0].astype(bool).sum()), "device_bytes_held": int(held)}
        if scan:
            # the scan launch alone, over the whole batch on an idle device: HIP events round 50 launches
            ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            st = streams[0]
            b.height_scan(0, n, stream=st.cuda_stream)
            torch.cuda.synchronize()
            with torch.cuda.stream(st):
                ev0.record()
                for _ in range(50):
                    b.height_scan(0, n, stream=st.cuda_stream)
                ev1.record()
            torch.cuda.synchronize()
            info["scan_launch_alone_us"] = 1000.0 * ev0.elapsed_time(ev1) / 50
            info["scan_points"] = int(b.dim(P.F_HEIGHT_SCAN))
            v = b.get(P.F_HEIGHT_SCAN)
            info["scan_value_range"] = [float(v.min()), float(v.max())]
        return info
    finally:
        b.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--only", choices=SETTINGS, default=None, help="one setting only (e.g. under a kernel trace, or on another build)")
    ap.add_argument("--parent-lib", default=None, help="another build of the library (CASSIE_LIB): its `shared` leg is run in a child process")
    a = ap.parse_args()
    model = Model("cassie_hfield")
    out = {"tool": "terrain_rate", "model": "cassie_hfield", "envs": a.envs, "substeps_per_launch": NSUB, "launches_per_region": a.launches,
           "warmup_launches": a.warmup, "terrains_in_the_bank": NTERRAIN,
           "mode": "CM_DRIVE_PD_SAFE, 50 fused substeps per launch, two env ranges on two streams, restarts on the benchmark's schedule (config 4)",
           "yardstick": "shared"}
    for name in SETTINGS:
        if a.only in (None, name):
            out[name] = regions(model, a.envs, name, a.launches, a.warmup, a.repeats)
    if a.parent_lib:
        cmd = [sys.executable, os.path.abspath(__file__), "--only", "shared", "--envs", str(a.envs), "--launches", str(a.launches),
               "--warmup", str(a.warmup), "--repeats", str(a.repeats)]
        r = subprocess.run(cmd, env=dict(os.environ, CASSIE_LIB=os.path.abspath(a.parent_lib)), capture_output=True, text=True, timeout=900)
        if r.returncode != 0:
            raise SystemExit("the parent build's leg failed:\n" + r.stdout + r.stderr)
        out["parent_shared"] = json.loads(r.stdout.strip().splitlines()[-1])["shared"]
        if "shared" in out:
            lo, hi, med = out["parent_shared"]["env_steps_per_s_min"], out["parent_shared"]["env_steps_per_s_max"], out["shared"]["env_steps_per_s_median"]
            out["shared_median_inside_the_parents_spread"] = bool(lo <= med <= hi)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
