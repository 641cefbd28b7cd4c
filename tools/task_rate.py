#!/usr/bin/env python3
"""What the task row per policy step costs config 2's loop -- 4096 cassie.xml envs, CM_DRIVE_PD_SAFE, 50 fused substeps per launch, the
batch as two env ranges on two streams with nothing joining them, restarts on bench.py's schedule -- in three legs that ALTERNATE in one
process on one box, fenced timed regions, ten each:

  loop          the loop alone, F_PD_PTARGET bound as the benchmark binds it and xfrc_applied uploaded as zeros (so that the step kernel
                is handed the applied forces in every leg).  THE YARDSTICK.
  task          the same plus one phys_batch_task per range and policy step, on the range's stream BEHIND its step launch: 21 columns
                (float32) -- a command group of three resampled every 100 .. 250 calls and resting with probability 0.1, a gait
                frequency, a clock with sin and cos and two trapezoid gates half a cycle apart, ten columns of a 240-frame reference
                table, and a push group of two into xfrc_applied (shown 2 calls of 150 .. 400, a few newtons).
  torch         the same row made with torch operations on the same streams: per-env timers and masked resampling with torch.rand, the
                phase accumulator, sin / cos, the gates, the gathered and interpolated table rows, the pushes written into a bound
                xfrc_applied tensor and cleared again.  What a user does today.

The pushes are kept to a few newtons so that the legs differ in what follows a step launch, not in what the step kernel meets.

--parent-lib PATH runs the `loop` leg alone in child processes, in the order parent, this build, this build, parent, against another
build of the library (the parent commit's) and against this one: like against like, one batch in a fresh process of its own, the regions
of a build's two runs pooled.  No stepping kernel changes with the task rows, so this build's median should lie inside the parent's
regions.

Also times the task call alone over the whole batch on an idle device.  Every region is recorded.  Prints one JSON line; `--out` also
writes it to a file.  Needs a GPU.

    python tools/task_rate.py [--envs 4096] [--launches 20] [--warmup 10] [--repeats 10] [--only NAME] [--out profiles/task_rate.json]
                              [--parent-lib PATH]
"""
import argparse
import json
import math
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
LEGS = ("loop", "task", "torch")
NREF, NFRAMES, PUSH_N = 10, 240, 5.0
CMD_LO, CMD_HI, P_REST, PUSH_LO, PUSH_HI, PUSH_HOLD = 100, 250, 0.1, 150, 400, 2
RATE, RATE_SCALE, DUTY, RAMP = 0.02, 0.01, 0.45, 0.1
# the row: vx vy yaw | freq | clock sin cos | gate gate | ten reference columns | push x, y
VX, FREQ, CLOCK, SIN, COS, GATE, REF, PUSH, NCOLS = 0, 3, 4, 5, 6, 7, 9, 19, 21


def task_columns(pod):
    cols = [P.task_sample(0.5, 1.0, CMD_LO, CMD_HI, p_rest=P_REST), P.task_sample(0.0, 0.3, CMD_LO, CMD_HI, p_rest=P_REST, group=0),
            P.task_sample(0.0, 0.5, CMD_LO, CMD_HI, p_rest=P_REST, group=0), P.task_sample(0.0, 1.0, 200, 500),
            P.task_phase(rate=RATE, rate_col=FREQ, rate_scale=RATE_SCALE), P.task_wave(CLOCK, P.TASK_SIN), P.task_wave(CLOCK, P.TASK_COS),
            P.task_wave(CLOCK, P.TASK_TRAPEZOID, duty=DUTY, ramp=RAMP), P.task_wave(CLOCK, P.TASK_TRAPEZOID, shift=0.5, duty=DUTY, ramp=RAMP)]
    cols += [P.task_table(CLOCK, j, shift=0.5 * (j >= NREF // 2)) for j in range(NREF)]
    cols += [P.task_sample(0.0, PUSH_N, PUSH_LO, PUSH_HI, hold=PUSH_HOLD, dfield=P.F_XFRC_APPLIED, dindex=6 + 0),
             P.task_sample(0.0, PUSH_N, PUSH_LO, PUSH_HI, hold=PUSH_HOLD, group=PUSH, dfield=P.F_XFRC_APPLIED, dindex=6 + 1)]
    assert len(cols) == NCOLS
    return cols


def reference_table():
    ph = 2.0 * math.pi * np.arange(NFRAMES)[:, None] / NFRAMES
    return bench.PD_OFFSET[None, :NREF] + 0.1 * np.sin(ph + np.arange(NREF)[None, :])


class Leg:
    """One batch running config 2's loop, with what its leg adds behind every range's step launch."""

    def __init__(self, model, n, leg):
        pod = model.pod
        self.leg, self.n, self.pod = leg, n, pod
        self.b = b = Batch(model, n)
        dev = torch.device("cuda")
        rng = np.random.default_rng(1)
        self.tgt = torch.from_numpy(bench.PD_OFFSET + rng.uniform(-0.3, 0.3, (n, 10))).to(dev)
        self.xfrc = torch.zeros((n, 6 * pod.nbody), dtype=torch.float64, device=dev)
        torch.cuda.synchronize()
        b.bind(P.F_PD_PTARGET, self.tgt.data_ptr())
        b.set(P.F_QPOS, np.tile(model.qpos_init(), (n, 1)))
        b.forward()
        sens0 = b.get(P.F_SENSORDATA, 0, 1)[0]
        b.set(P.F_PD_KP, np.tile(bench.PD_KP, (n, 1)))
        b.set(P.F_PD_KD, np.tile(bench.PD_KD, (n, 1)))
        b.set_drive_mode(P.DRIVE_PD_SAFE)
        self.init_row = torch.from_numpy(np.concatenate([model.qpos_init(), sens0])).cuda()
        b.bind(P.F_XFRC_APPLIED, self.xfrc.data_ptr())
        self.rows = torch.zeros((n, NCOLS), dtype=torch.float32, device=dev)
        table = reference_table()
        if leg == "task":
            b.set_task_table(table)
            b.configure_task(task_columns(pod), dtype=np.float32, seed=1)
            b.bind_task_rows(self.rows.data_ptr(), NCOLS)
        if leg == "torch":
            self.table = torch.from_numpy(table).to(dev)
            self.left = torch.zeros((3, n), dtype=torch.int32, device=dev)          # the timers of the command, the frequency, the push
            self.age = torch.zeros(n, dtype=torch.int32, device=dev)
            self.held = torch.zeros((n, 6), dtype=torch.float64, device=dev)        # vx vy yaw | freq | push x, y
            self.phi = torch.zeros(n, dtype=torch.float64, device=dev)
            self.center = torch.tensor([0.5, 0.0, 0.0], dtype=torch.float64, device=dev)
            self.half = torch.tensor([1.0, 0.3, 0.5], dtype=torch.float64, device=dev)
            self.shift = torch.tensor([0.0] * (NREF // 2) + [0.5] * (NREF - NREF // 2), dtype=torch.float64, device=dev)
            self.tcol = torch.arange(NREF, device=dev)
        b.sync()
        torch.cuda.synchronize()
        self.streams, half = [torch.cuda.Stream(), torch.cuda.Stream()], n // 2
        self.ranges = [(0, half), (half, n - half)]
        self.policy_step = 0
        self.rates = []

    def torch_task(self, e0, cnt):
        """The row of the range as a user makes it today (on the current stream)."""
        s = slice(e0, e0 + cnt)
        dev = self.rows.device
        left, held = self.left[:, s], self.held[s]
        due = left <= 0
        # the command: a new period, a rest with probability P_REST, three uniform values
        period = torch.randint(CMD_LO, CMD_HI + 1, (cnt,), dtype=torch.int32, device=dev)
        rest = torch.rand(cnt, device=dev) < P_REST
        cmd = self.center + self.half * (2.0 * torch.rand((cnt, 3), dtype=torch.float64, device=dev) - 1.0)
        cmd = torch.where(rest[:, None], torch.zeros_like(cmd), cmd)
        held[:, 0:3] = torch.where(due[0][:, None], cmd, held[:, 0:3])
        left[0] = torch.where(due[0], period, left[0])
        # the frequency
        held[:, 3] = torch.where(due[1], 2.0 * torch.rand(cnt, dtype=torch.float64, device=dev) - 1.0, held[:, 3])
        left[1] = torch.where(due[1], torch.randint(200, 501, (cnt,), dtype=torch.int32, device=dev), left[1])
        # the push: shown PUSH_HOLD calls of its period
        push = PUSH_N * (2.0 * torch.rand((cnt, 2), dtype=torch.float64, device=dev) - 1.0)
        held[:, 4:6] = torch.where(due[2][:, None], push, held[:, 4:6])
        self.age[s] = torch.where(due[2], torch.zeros_like(self.age[s]), self.age[s])
        left[2] = torch.where(due[2], torch.randint(PUSH_LO, PUSH_HI + 1, (cnt,), dtype=torch.int32, device=dev), left[2])
        shown = torch.where((self.age[s] < PUSH_HOLD)[:, None], held[:, 4:6], torch.zeros_like(held[:, 4:6]))
        self.xfrc[s, 6:8] = shown
        left -= 1
        self.age[s] += 1
        # the clock, its waveforms and the reference row
        phi = self.phi[s] + (RATE + RATE_SCALE * held[:, 3])
        phi = phi - torch.floor(phi)
        self.phi[s] = phi
        ang = 2.0 * math.pi * phi

        def gate(theta):
            return (theta / RAMP).clamp(0.0, 1.0) - ((theta - DUTY) / RAMP).clamp(0.0, 1.0)

        other = phi + 0.5
        other = other - torch.floor(other)
        theta = phi[:, None] + self.shift
        theta = theta - torch.floor(theta)
        x = theta * NFRAMES
        i = x.floor().long().clamp(0, NFRAMES - 1)
        fr = x - i
        j = (i + 1) % NFRAMES
        ta, tb = self.table[i, self.tcol], self.table[j, self.tcol]
        ref = ta + fr * (tb - ta)
        row = torch.cat([held[:, 0:4], phi[:, None], torch.sin(ang)[:, None], torch.cos(ang)[:, None], gate(phi)[:, None], gate(other)[:, None], ref, shown], dim=1)
        self.rows[s] = row.float()

    def launch(self):
        b, p = self.b, self.policy_step
        self.policy_step += 1
        for (first, cnt), st in zip(self.ranges, self.streams):
            r0, k = bench.rows_of_group_in_range(bench.restart_group(p), 0, first, cnt)
            if k:
                b.reset_envs(r0, bench.NGROUP, k, self.init_row.data_ptr(), self.init_row.data_ptr() + 8 * self.pod.nq, st.cuda_stream)
            b.step_range(first, cnt, NSUB, st.cuda_stream)
            if self.leg == "task":
                b.task(first, cnt, stream=st.cuda_stream)
            elif self.leg == "torch":
                with torch.cuda.stream(st):
                    self.torch_task(first, cnt)

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
            out["columns"] = NCOLS
            out["finite_rows"] = int(np.isfinite(rows).all(axis=1).sum())
            out["rows_with_a_command"] = int((rows[:, VX: VX + 3] != 0).any(axis=1).sum())
            out["largest_sin2_plus_cos2_minus_1"] = float(np.abs(rows[:, SIN].astype(np.float64) ** 2 + rows[:, COS].astype(np.float64) ** 2 - 1.0).max())
            out["envs_pushed_now"] = int((self.xfrc.cpu().numpy()[:, 6:8] != 0).any(axis=1).sum())
        if self.leg == "task":
            out["task_launches"] = self.b.task_launches()
            out["row"] = {"columns": NCOLS, "dtype": "float32", "bytes_per_env": 4 * NCOLS, "state_bytes_per_env": (8 + 12) * NCOLS, "table_frames": NFRAMES}
            # the call alone over the whole batch on an idle device: device events round 20 calls
            ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            st = self.streams[0]
            self.b.task(0, self.n, stream=st.cuda_stream)
            torch.cuda.synchronize()
            with torch.cuda.stream(st):
                ev0.record()
                for _ in range(20):
                    self.b.task(0, self.n, stream=st.cuda_stream)
                ev1.record()
            torch.cuda.synchronize()
            out["task_call_alone_us"] = 1000.0 * ev0.elapsed_time(ev1) / 20
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
    ap.add_argument("--parent-lib", default=None, help="another build of the library (the parent commit's): its `loop` leg, in child processes")
    a = ap.parse_args()
    out = {"tool": "task_rate", "model": "cassie", "envs": a.envs, "substeps_per_launch": NSUB, "launches_per_region": a.launches,
           "warmup_launches": a.warmup, "regions_per_leg": a.repeats,
           "mode": "CM_DRIVE_PD_SAFE, 50 fused substeps per launch, two env ranges on two streams, restarts on the benchmark's schedule (config 2); "
                   "the legs alternate region by region in one process; the task row of a range behind its step launch",
           "yardstick": "loop"}
    if a.parent_lib:
        # (first, in fresh processes of their own: one library per process; this process has not touched the GPU yet)
        def alone(lib):
            cmd = [sys.executable, os.path.abspath(__file__), "--only", "loop", "--envs", str(a.envs), "--launches", str(a.launches),
                   "--warmup", str(a.warmup), "--repeats", str(a.repeats)]
            env = dict(os.environ, CASSIE_LIB=os.path.abspath(lib)) if lib else {k: v for k, v in os.environ.items() if k != "CASSIE_LIB"}
            r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=900)
            if r.returncode != 0:
                sys.exit("a child leg failed:\n" + r.stderr[-2000:])
            return json.loads(r.stdout.strip().splitlines()[-1])["loop"]

        def pooled(runs):
            r = [v for run in runs for v in run["regions"]]
            return {"env_steps_per_s_median": float(np.median(r)), "env_steps_per_s_min": float(min(r)), "env_steps_per_s_max": float(max(r)),
                    "spread_percent_of_median": 100.0 * (max(r) - min(r)) / float(np.median(r)), "regions": r,
                    "run_medians": [run["env_steps_per_s_median"] for run in runs], "envs_with_warnings": sum(run["envs_with_warnings"] for run in runs)}

        runs = [alone(lib) for lib in (a.parent_lib, None, None, a.parent_lib)]
        out["parent_loop"], out["loop_alone"] = pooled([runs[0], runs[3]]), pooled([runs[1], runs[2]])
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
        out["loop_spread_percent"] = out["loop"]["spread_percent_of_median"]
    if "task" in out and "torch" in out:
        one, many = out["task"]["env_steps_per_s_median"], out["torch"]["env_steps_per_s_median"]
        out["cheaper_task_leg"] = "task" if one > many else "torch"
        out["task_loses_less_than_torch"] = bool(one > many)
        out["largest_spread_of_a_leg_percent"] = max(out[name]["spread_percent_of_median"] for name in LEGS if name in out)
        if "loop" in out:
            out["task_costs_no_more_than_the_loops_spread"] = bool(out["task"]["cost_of_the_loop_percent"] <= out["loop_spread_percent"])
            out["difference_of_the_task_legs_percent_of_loop"] = 100.0 * abs(one - many) / out["loop"]["env_steps_per_s_median"]
    if "parent_loop" in out:
        par, own = out["parent_loop"], out["loop_alone"]
        out["loop_median_over_parent_median"] = own["env_steps_per_s_median"] / par["env_steps_per_s_median"]
        out["loop_median_within_the_parents_regions"] = bool(par["env_steps_per_s_min"] <= own["env_steps_per_s_median"] <= par["env_steps_per_s_max"])
        out["difference_of_medians_percent"] = 100.0 * abs(out["loop_median_over_parent_median"] - 1.0)
        out["parents_spread_percent"] = par["spread_percent_of_median"]
        out["unused_the_feature_costs_less_than_the_parents_spread"] = bool(out["difference_of_medians_percent"] < par["spread_percent_of_median"])
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
