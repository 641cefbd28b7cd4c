#!/usr/bin/env python3
"""What placed restarts cost config 4's loop -- 4096 cassie_hfield.xml envs, CM_DRIVE_PD_SAFE, 50 fused substeps per launch, the batch as
two env ranges on two streams, a bank of 64 terrains, phys_batch_end_episodes per range per policy step with max_steps = bench.NGROUP
and the step counters started at e % NGROUP (the benchmark's restart schedule) -- in three settings, fenced timed regions:

  unplaced    restarts copy the bank row (the loop as it was).  THE YARDSTICK; `--parent-lib` runs this leg again, in a child process,
              on another build of the library (the parent commit's: CASSIE_LIB), in the same session.
  placed      phys_batch_place_configure without a footprint: a per-env shift and yaw, no ground lookup.
  footprint   a 9-point footprint (3 x 3, 0.15 m apart) and next terrains bound: a terrain change and a ground lookup per restart.

Every leg has a batch of its own; the legs' regions ALTERNATE (leg A, B, C, A, B, C, ...) after a warm-up of each, so that a drift of
the machine meets all of them alike.  The spawn poses keep the feet on the flat start patch all terrains share (|dx|, |dy| <= 0.02 m, any
yaw), so the placed legs step the physics of the unplaced one turned about the vertical.  Prints one JSON line: the regions of each leg
(env-steps per second), their medians, and per leg the time of the end_episodes launch ALONE over the whole batch on an idle device with
every env restarting (`restart_launch_alone_us`: HIP events round 50 launches).  Needs a GPU.

    python tools/placement_rate.py [--envs 4096] [--launches 20] [--warmup 10] [--repeats 10] [--only NAME] [--parent-lib PATH]
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
import torch  # noqa: E402
from cassie_amd import Batch, Model  # noqa: E402
from cassie_amd import phys as P  # noqa: E402

NSUB = bench.HOLD
LEGS = ("unplaced", "placed", "footprint")
NTERRAIN = 64


def terrain(seed):
    h = np.random.default_rng(seed).random((200, 200)).astype(np.float32)
    h[95:105, 95:105] = 0
    return h


class Leg:
    """One setting's batch and its loop."""

    def __init__(self, model, n, name):
        pod = model.pod
        self.n, self.name = n, name
        b = self.b = Batch(model, n)
        rng = np.random.default_rng(3)
        b.set_hfield_bank(np.stack([terrain(99 + k) for k in range(NTERRAIN)]))
        b.set_terrain(rng.integers(0, NTERRAIN, n).astype(np.int32))
        q0 = model.qpos_init()
        b.set(P.F_QPOS, np.tile(q0, (n, 1)))
        b.forward()
        b.set(P.F_PD_KP, np.tile(bench.PD_KP, (n, 1)))
        b.set(P.F_PD_KD, np.tile(bench.PD_KD, (n, 1)))
        b.set(P.F_PD_PTARGET, bench.PD_OFFSET + np.random.default_rng(1).uniform(-0.3, 0.3, (n, 10)))
        b.set_drive_mode(P.DRIVE_PD_SAFE)
        b.enable_episodes(max_steps=bench.NGROUP)
        b.set_reset_bank(b.make_reset_bank(q0[None]))
        self.keep = [torch.from_numpy((np.arange(n) % bench.NGROUP).astype(np.int32)).cuda()]
        b.bind_episode(P.EP_STEPS, self.keep[0].data_ptr())
        if name != "unplaced":
            pts = None
            if name == "footprint":
                pts = np.array([[0.15 * i, 0.15 * j] for i in (-1, 0, 1) for j in (-1, 0, 1)])
                self.keep.append(torch.from_numpy(rng.integers(0, NTERRAIN, n).astype(np.int32)).cuda())
            # the rows stand on the flat start patch: elevation 0 of the height-field geom
            b.configure_placement(int(pod.root_body[0]), pts, float(pod.geom_pos[pod.hfield_geom][2]))
            b.set_placement(np.stack([rng.uniform(-0.02, 0.02, n), rng.uniform(-0.02, 0.02, n), np.zeros(n), rng.uniform(-np.pi, np.pi, n)], axis=1))
            if name == "footprint":
                b.bind_placement(P.PLACE_NEXT_TERRAIN, self.keep[1].data_ptr())
        b.sync()
        torch.cuda.synchronize()
        self.streams = [torch.cuda.Stream(), torch.cuda.Stream()]
        half = n // 2
        self.ranges = [(0, half), (half, n - half)]
        self.regions = []

    def launch(self):
        for (first, cnt), st in zip(self.ranges, self.streams):
            self.b.step_range(first, cnt, NSUB, st.cuda_stream)
            self.b.end_episodes(first, cnt, True, stream=st.cuda_stream)

    def region(self, launches):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(launches):
            self.launch()
        torch.cuda.synchronize()
        self.regions.append(self.n * NSUB * launches / (time.perf_counter() - t0))

    def launch_alone_us(self, reps=50):
        """The end_episodes launch over the whole batch with every env forced to restart, on an idle device."""
        force = torch.ones(self.n, dtype=torch.int32, device="cuda")
        st = self.streams[0]
        ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        self.b.end_episodes(0, self.n, True, force_ptr=force.data_ptr(), stream=st.cuda_stream)
        torch.cuda.synchronize()
        with torch.cuda.stream(st):
            ev0.record()
            for _ in range(reps):
                self.b.end_episodes(0, self.n, True, force_ptr=force.data_ptr(), stream=st.cuda_stream)
            ev1.record()
        torch.cuda.synchronize()
        return 1000.0 * ev0.elapsed_time(ev1) / reps

    def info(self):
        done, reason, steps, count, _ = self.b.episodes()
        out = {"env_steps_per_s_median": float(np.median(self.regions)), "env_steps_per_s_min": float(min(self.regions)),
               "env_steps_per_s_max": float(max(self.regions)), "regions": self.regions,
               "envs_with_warnings": int(self.b.warnings()[0].astype(bool).sum()), "episodes_ended": int(count.sum())}
        if self.name != "unplaced":
            g = self.b.placement_ground()
            out["ground_found_range"] = [float(g.min()), float(g.max())]
        out["restart_launch_alone_us"] = self.launch_alone_us()
        return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--only", choices=LEGS, default=None, help="one leg only (e.g. under a kernel trace, or on another build)")
    ap.add_argument("--parent-lib", default=None, help="another build of the library (CASSIE_LIB): its `unplaced` leg is run in a child process")
    a = ap.parse_args()
    model = Model("cassie_hfield")
    out = {"tool": "placement_rate", "model": "cassie_hfield", "envs": a.envs, "substeps_per_launch": NSUB, "launches_per_region": a.launches,
           "warmup_launches": a.warmup, "terrains_in_the_bank": NTERRAIN,
           "mode": "CM_DRIVE_PD_SAFE, 50 fused substeps per launch, two env ranges on two streams, end_episodes per range per policy step "
                   "with max_steps = %d (config 4's loop); the legs' regions alternate" % bench.NGROUP,
           "yardstick": "unplaced"}
    legs = [Leg(model, a.envs, name) for name in LEGS if a.only in (None, name)]
    try:
        for leg in legs:
            for _ in range(a.warmup):
                leg.launch()
        torch.cuda.synchronize()
        for _ in range(a.repeats):
            for leg in legs:
                leg.region(a.launches)
        for leg in legs:
            out[leg.name] = leg.info()
    finally:
        for leg in legs:
            leg.b.close()
    if a.parent_lib:
        cmd = [sys.executable, os.path.abspath(__file__), "--only", "unplaced", "--envs", str(a.envs), "--launches", str(a.launches),
               "--warmup", str(a.warmup), "--repeats", str(a.repeats)]
        r = subprocess.run(cmd, env=dict(os.environ, CASSIE_LIB=os.path.abspath(a.parent_lib)), capture_output=True, text=True, timeout=900)
        if r.returncode != 0:
            raise SystemExit("the parent build's leg failed:\n" + r.stdout + r.stderr)
        out["parent_unplaced"] = json.loads(r.stdout.strip().splitlines()[-1])["unplaced"]
        if "unplaced" in out:
            lo, hi, med = out["parent_unplaced"]["env_steps_per_s_min"], out["parent_unplaced"]["env_steps_per_s_max"], out["unplaced"]["env_steps_per_s_median"]
            out["unplaced_median_inside_the_parents_spread"] = bool(lo <= med <= hi)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
