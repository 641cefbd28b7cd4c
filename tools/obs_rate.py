#!/usr/bin/env python3
"""What the observation row per policy step costs config 2's loop -- 4096 cassie.xml envs, CM_DRIVE_PD_SAFE, 50 fused substeps per launch,
the batch as two env ranges on two streams with nothing joining them, restarts on bench.py's schedule -- in three legs that ALTERNATE in
one process on one box, fenced timed regions, ten each:

  loop          the loop alone.  THE YARDSTICK.
  observe       the same plus one phys_batch_obs per range and policy step, on the range's stream: a row of 85 columns x 4 frames in
                float32 -- 28 joint positions and 26 joint velocities with noise, the 13 IMU sensor values with noise, the projected
                gravity, the base velocity in the body frame and 12 columns of the caller's input.
  torch         the same row assembled with torch operations on the same streams, from the same fields bound to torch tensors: slices, a
                quaternion rotation, torch.rand noise, scale, clamp, the cast and a roll of the history.  What a user does today.

In every leg qpos, qvel and sensordata are bound to torch tensors (dense rows), so the legs differ in what follows a step launch alone.

--parent-lib PATH runs the `loop` leg once more in a child process against another build of the library (the parent commit's): no
stepping kernel changes with the observation rows, so this build's `loop` median should differ from the parent's by no more than the
spread of a leg's own regions.

Also times the observe call alone over the whole batch on an idle device.  Every region is recorded.  Prints one JSON line; `--out` also
writes it to a file.  Needs a GPU.

    python tools/obs_rate.py [--envs 4096] [--launches 20] [--warmup 10] [--repeats 10] [--only NAME] [--out profiles/obs_rate.json]
                             [--parent-lib PATH]
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
LEGS = ("loop", "observe", "torch")
HISTORY, NINPUT, IMU0, NIMU = 4, 12, 16, 13
NOISE_Q, NOISE_V, NOISE_IMU = 0.01, 0.1, 0.02


def obs_terms(pod):
    return [P.obs_copy(P.F_QPOS, 7, pod.nq - 7, noise=NOISE_Q), P.obs_copy(P.F_QVEL, 6, pod.nv - 6, scale=0.1, noise=NOISE_V),
            P.obs_copy(P.F_SENSORDATA, IMU0, NIMU, noise=NOISE_IMU, lo=-50.0, hi=50.0),
            P.obs_rot_inv(P.OBS_CONST, 0, P.F_QPOS, 3, vec=(0.0, 0.0, -1.0)), P.obs_rot_inv(P.F_QVEL, 0, P.F_QPOS, 3),
            P.obs_copy(P.OBS_INPUT, 0, NINPUT)]


class Leg:
    """One batch running config 2's loop, with what its leg adds behind every range's step launch."""

    def __init__(self, model, n, leg):
        pod = model.pod
        self.leg, self.n, self.pod = leg, n, pod
        self.b = b = Batch(model, n)
        dev = torch.device("cuda")
        self.qpos = torch.zeros((n, pod.nq), dtype=torch.float64, device=dev)
        self.qvel = torch.zeros((n, pod.nv), dtype=torch.float64, device=dev)
        self.sens = torch.zeros((n, pod.nsensordata), dtype=torch.float64, device=dev)
        torch.cuda.synchronize()
        for f, t in ((P.F_QPOS, self.qpos), (P.F_QVEL, self.qvel), (P.F_SENSORDATA, self.sens)):
            b.bind(f, t.data_ptr())
        b.set(P.F_QPOS, np.tile(model.qpos_init(), (n, 1)))
        b.forward()
        sens0 = b.get(P.F_SENSORDATA, 0, 1)[0]
        b.set(P.F_PD_KP, np.tile(bench.PD_KP, (n, 1)))
        b.set(P.F_PD_KD, np.tile(bench.PD_KD, (n, 1)))
        b.set(P.F_PD_PTARGET, bench.PD_OFFSET + np.random.default_rng(1).uniform(-0.3, 0.3, (n, 10)))
        b.set_drive_mode(P.DRIVE_PD_SAFE)
        self.init_row = torch.from_numpy(np.concatenate([model.qpos_init(), sens0])).cuda()
        self.ncols = (pod.nq - 7) + (pod.nv - 6) + NIMU + 3 + 3 + NINPUT
        self.inp = torch.rand((n, NINPUT), dtype=torch.float32, device=dev)
        self.rows = torch.zeros((n, HISTORY, self.ncols), dtype=torch.float32, device=dev)
        if leg == "observe":
            b.configure_obs(obs_terms(pod), history=HISTORY, dtype=np.float32, seed=1)
            assert b.obs_dim() == (self.ncols, HISTORY, HISTORY * self.ncols)
            b.bind_obs(self.rows.data_ptr())
            b.bind_obs_input(self.inp.data_ptr(), NINPUT, NINPUT, torch.float32)
        if leg == "torch":
            self.amp = torch.cat([torch.full((pod.nq - 7,), NOISE_Q), torch.full((pod.nv - 6,), NOISE_V), torch.full((NIMU,), NOISE_IMU),
                                  torch.zeros(6 + NINPUT)]).to(dev, torch.float64)
            self.scale = torch.cat([torch.ones(pod.nq - 7), torch.full((pod.nv - 6,), 0.1), torch.ones(NIMU + 6 + NINPUT)]).to(dev, torch.float64)
            self.down = torch.tensor([0.0, 0.0, -1.0], dtype=torch.float64, device=dev)
            self.first = True
        b.sync()
        torch.cuda.synchronize()
        self.streams, half = [torch.cuda.Stream(), torch.cuda.Stream()], n // 2
        self.ranges = [(0, half), (half, n - half)]
        self.policy_step = 0
        self.rates = []

    def torch_observation(self, e0, cnt):
        """The row of the range as a user assembles it today (on the current stream)."""
        pod = self.pod
        q, v, s = self.qpos[e0: e0 + cnt], self.qvel[e0: e0 + cnt], self.sens[e0: e0 + cnt]
        w, x, y, z = q[:, 3], q[:, 4], q[:, 5], q[:, 6]
        R = torch.stack([w * w + x * x - y * y - z * z, 2 * (x * y - w * z), 2 * (x * z + w * y),
                         2 * (x * y + w * z), w * w - x * x + y * y - z * z, 2 * (y * z - w * x),
                         2 * (x * z - w * y), 2 * (y * z + w * x), w * w - x * x - y * y + z * z], dim=1).reshape(cnt, 3, 3)
        grav = torch.matmul(R.transpose(1, 2), self.down)
        vel = torch.matmul(R.transpose(1, 2), v[:, :3].unsqueeze(2)).squeeze(2)
        frame = torch.cat([q[:, 7:], v[:, 6:], s[:, IMU0: IMU0 + NIMU].clamp(-50.0, 50.0), grav, vel, self.inp[e0: e0 + cnt].double()], dim=1)
        xi = torch.rand((cnt, self.ncols), dtype=torch.float64, device=frame.device) * 2.0 - 1.0
        frame = ((frame + self.amp * xi) * self.scale).float()
        rows = self.rows[e0: e0 + cnt]
        if self.first:
            rows[:] = frame.unsqueeze(1)
        else:
            rows[:, 1:] = rows[:, :-1].clone()
            rows[:, 0] = frame

    def launch(self):
        b, p = self.b, self.policy_step
        self.policy_step += 1
        for (first, cnt), st in zip(self.ranges, self.streams):
            r0, k = bench.rows_of_group_in_range(bench.restart_group(p), 0, first, cnt)
            if k:
                b.reset_envs(r0, bench.NGROUP, k, self.init_row.data_ptr(), self.init_row.data_ptr() + 8 * self.pod.nq, st.cuda_stream)
            b.step_range(first, cnt, NSUB, st.cuda_stream)
            if self.leg == "observe":
                b.observe(first, cnt, stream=st.cuda_stream)
            elif self.leg == "torch":
                with torch.cuda.stream(st):
                    self.torch_observation(first, cnt)
        if self.leg == "torch":
            self.first = False

    def region(self, launches):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(launches):
            self.launch()
        torch.cuda.synchronize()
        self.rates.append(self.n * NSUB * launches / (time.perf_counter() - t0))

    def report(self):
        r = self.rates
        out = {"env_steps_per_s_median": float(np.median(r)), "env_steps_per_s_min": float(min(r)), "env_steps_per_s_max": float(max(r)),
               "spread_percent_of_median": 100.0 * (max(r) - min(r)) / float(np.median(r)), "regions": r,
               "envs_with_warnings": int(self.b.warnings()[0].astype(bool).sum())}
        if self.leg != "loop":
            rows = self.rows.cpu().numpy()
            out["row"] = {"columns": self.ncols, "frames": HISTORY, "dtype": "float32", "bytes_per_env": 4 * HISTORY * self.ncols}
            out["finite_rows"] = int(np.isfinite(rows).all(axis=(1, 2)).sum())
            out["rows_whose_frames_differ"] = int((rows[:, 0] != rows[:, 1]).any(axis=1).sum())
        if self.leg == "observe":
            out["obs_launches"] = self.b.obs_launches()
            # the call alone over the whole batch on an idle device: device events round 20 calls
            ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            st = self.streams[0]
            self.b.observe(0, self.n, stream=st.cuda_stream)
            torch.cuda.synchronize()
            with torch.cuda.stream(st):
                ev0.record()
                for _ in range(20):
                    self.b.observe(0, self.n, stream=st.cuda_stream)
                ev1.record()
            torch.cuda.synchronize()
            out["observe_call_alone_us"] = 1000.0 * ev0.elapsed_time(ev1) / 20
        return out

    def close(self):
        self.b.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--only", choices=list(LEGS), default=None, help="one leg only")
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    ap.add_argument("--parent-lib", default=None, help="another build of the library (the parent commit's): its `loop` leg, in a child process")
    a = ap.parse_args()
    out = {"tool": "obs_rate", "model": "cassie", "envs": a.envs, "substeps_per_launch": NSUB, "launches_per_region": a.launches,
           "warmup_launches": a.warmup, "regions_per_leg": a.repeats,
           "mode": "CM_DRIVE_PD_SAFE, 50 fused substeps per launch, two env ranges on two streams, restarts on the benchmark's schedule (config 2); "
                   "the legs alternate region by region in one process; an observation per range behind its step launch",
           "yardstick": "loop"}
    if a.parent_lib:
        # (first, in a process of its own: one library per process; this process has not touched the GPU yet)
        cmd = [sys.executable, os.path.abspath(__file__), "--only", "loop", "--envs", str(a.envs), "--launches", str(a.launches),
               "--warmup", str(a.warmup), "--repeats", str(a.repeats)]
        r = subprocess.run(cmd, env=dict(os.environ, CASSIE_LIB=os.path.abspath(a.parent_lib)), capture_output=True, text=True, timeout=900)
        if r.returncode != 0:
            sys.exit("the --parent-lib leg failed:\n" + r.stderr[-2000:])
        out["parent_loop"] = json.loads(r.stdout.strip().splitlines()[-1])["loop"]
    model = Model("cassie")
    legs = [Leg(model, a.envs, name) for name in LEGS if a.only in (None, name)]
    try:
        for leg in legs:
            for _ in range(a.warmup):
                leg.launch()
        for _ in range(a.repeats):
            for leg in legs:
                leg.region(a.launches)
        for leg in legs:
            out[leg.leg] = leg.report()
    finally:
        for leg in legs:
            leg.close()
    if "loop" in out:
        base = out["loop"]["env_steps_per_s_median"]
        for name in LEGS[1:]:
            if name in out:
                out[name]["cost_of_the_loop_percent"] = 100.0 * (1.0 - out[name]["env_steps_per_s_median"] / base)
    if "observe" in out and "torch" in out:
        out["observe_costs_less_than_torch"] = bool(out["observe"]["env_steps_per_s_median"] > out["torch"]["env_steps_per_s_median"])
    if "parent_loop" in out and "loop" in out:
        par, own = out["parent_loop"], out["loop"]
        out["loop_median_over_parent_median"] = own["env_steps_per_s_median"] / par["env_steps_per_s_median"]
        out["loop_median_within_the_parents_regions"] = bool(par["env_steps_per_s_min"] <= own["env_steps_per_s_median"] <= par["env_steps_per_s_max"])
        out["difference_of_medians_percent"] = 100.0 * abs(out["loop_median_over_parent_median"] - 1.0)
        out["larger_spread_of_the_two_legs_percent"] = max(par["spread_percent_of_median"], own["spread_percent_of_median"])
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
