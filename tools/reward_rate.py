#!/usr/bin/env python3
"""What the reward per policy step costs config 2's loop -- 4096 cassie.xml envs, CM_DRIVE_PD_SAFE, 50 fused substeps per launch, the batch
as two env ranges on two streams with nothing joining them, restarts on bench.py's schedule -- in three legs that ALTERNATE in one process
on one box, fenced timed regions, ten each:

  loop          the loop alone.  THE YARDSTICK.
  reward        the same plus one phys_batch_reward per range and policy step, on the range's stream: a 12-term locomotion reward on the
                state and the caller's input (sources that need no other launch) -- the base velocity in the body frame against the
                command, the angular velocity, the orientation, the height through a deadband, ten joints against a reference pose, the
                joint velocities, the action rate and size, two clock-gated terms, an IMU term and the projected gravity -- with the
                term rows and the episode returns.
  torch         the same reward written with torch operations on the same streams, from the same fields bound to torch tensors.  What a
                user does today.

In every leg qpos, qvel and sensordata are bound to torch tensors (dense rows), so the legs differ in what follows a step launch alone.

--parent-lib PATH runs the `loop` leg alone in child processes, in the order parent, this build, this build, parent, against another
build of the library (the parent commit's) and against this one: like against like, one batch in a process of its own, the regions of a
build's two runs pooled.  No stepping kernel changes with the reward rows, so this build's median should lie inside the parent's regions.

Also times the reward call alone over the whole batch on an idle device.  Every region is recorded.  Prints one JSON line; `--out` also
writes it to a file.  Needs a GPU.

    python tools/reward_rate.py [--envs 4096] [--launches 20] [--warmup 10] [--repeats 10] [--only NAME] [--out profiles/reward_rate.json]
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
LEGS = ("loop", "reward", "torch")
# the input's columns: the commanded velocity | two clock coefficients | the reference pose of ten joints | the action | the previous action
IN_CMD, IN_CLOCK, IN_POSE, IN_ACT, IN_PREV, NINPUT = 0, 3, 5, 15, 25, 35
IMU_GYRO = 16 + 4          # (sensordata: the IMU's block starts at 16 with the orientation)
HEIGHT, DEAD, LO, HI = 0.9, 0.02, -1.0, 1.0


def reward_terms():
    IN, EXP = P.REW_INPUT, P.REW_EXP
    return [P.rew_rot_inv(P.F_QVEL, 0, P.F_QPOS, 3, tfield=IN, tindex=IN_CMD, shape=EXP, k=4.0, weight=0.2),
            P.rew_vec(P.F_QVEL, 3, 3, shape=EXP, k=0.5, weight=0.1),
            P.rew_quat(P.F_QPOS, 3, shape=EXP, k=5.0, weight=0.15),
            P.rew_vec(P.F_QPOS, 2, 1, target=HEIGHT, dead=DEAD, norm=P.REW_SUMABS, shape=EXP, k=10.0, weight=0.1),
            P.rew_vec(P.F_QPOS, 7, 10, tfield=IN, tindex=IN_POSE, shape=EXP, k=2.0, weight=0.15),
            P.rew_vec(P.F_QVEL, 6, 26, weight=-1e-4),
            P.rew_vec(IN, IN_ACT, 10, tfield=IN, tindex=IN_PREV, weight=-0.01),
            P.rew_vec(IN, IN_ACT, 10, norm=P.REW_SUMABS, weight=-0.001),
            P.rew_vec(P.F_QVEL, 12, 3, root=True, shape=EXP, k=1.0, weight=0.05, gate=(IN, IN_CLOCK)),
            P.rew_vec(P.F_QVEL, 25, 3, root=True, shape=EXP, k=1.0, weight=0.05, gate=(IN, IN_CLOCK + 1)),
            P.rew_vec(P.F_SENSORDATA, IMU_GYRO, 3, norm=P.REW_MAXABS, shape=P.REW_RATIONAL, k=0.1, weight=0.05),
            P.rew_rot_inv(P.REW_CONST, 0, P.F_QPOS, 3, vec=(0.0, 0.0, -1.0), norm=P.REW_SUMABS, weight=-0.02)]


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
        self.nterms = len(reward_terms())
        torch.manual_seed(1)               # (the same input in every leg: the two reward legs then report the same rewards)
        self.inp = torch.rand((n, NINPUT), dtype=torch.float32, device=dev)
        self.rew = torch.zeros(n, dtype=torch.float32, device=dev)
        self.rows = torch.zeros((n, self.nterms), dtype=torch.float32, device=dev)
        self.ret = torch.zeros(n, dtype=torch.float64, device=dev)
        self.fin = torch.zeros(n, dtype=torch.float64, device=dev)
        self.done = torch.zeros(n, dtype=torch.int32, device=dev)          # (stands for the EP_DONE words: nobody ends an episode here)
        if leg == "reward":
            b.configure_rewards(reward_terms(), dtype=np.float32, lo=LO, hi=HI)
            b.bind_rewards(self.rew.data_ptr())
            b.bind_reward_terms(self.rows.data_ptr())
            b.bind_reward_input(self.inp.data_ptr(), NINPUT, NINPUT, torch.float32)
        if leg == "torch":
            self.down = torch.tensor([0.0, 0.0, -1.0], dtype=torch.float64, device=dev)
            self.unit = torch.tensor([1.0, 0.0, 0.0, 0.0], dtype=torch.float64, device=dev)
        b.sync()
        torch.cuda.synchronize()
        self.streams, half = [torch.cuda.Stream(), torch.cuda.Stream()], n // 2
        self.ranges = [(0, half), (half, n - half)]
        self.policy_step = 0
        self.rates = []

    def torch_reward(self, e0, cnt):
        """The reward of the range as a user writes it today (on the current stream)."""
        q, v, s = self.qpos[e0: e0 + cnt], self.qvel[e0: e0 + cnt], self.sens[e0: e0 + cnt]
        u = self.inp[e0: e0 + cnt].double()
        w, x, y, z = q[:, 3], q[:, 4], q[:, 5], q[:, 6]
        R = torch.stack([w * w + x * x - y * y - z * z, 2 * (x * y - w * z), 2 * (x * z + w * y),
                         2 * (x * y + w * z), w * w - x * x + y * y - z * z, 2 * (y * z - w * x),
                         2 * (x * z - w * y), 2 * (y * z + w * x), w * w - x * x - y * y + z * z], dim=1).reshape(cnt, 3, 3)
        vel = torch.matmul(R.transpose(1, 2), v[:, :3].unsqueeze(2)).squeeze(2)
        grav = torch.matmul(R.transpose(1, 2), self.down)
        d = (q[:, 3:7] * self.unit).sum(1)
        terms = torch.stack([
            0.2 * torch.exp(-4.0 * ((vel - u[:, IN_CMD: IN_CMD + 3]) ** 2).sum(1)),
            0.1 * torch.exp(-0.5 * (v[:, 3:6] ** 2).sum(1)),
            0.15 * torch.exp(-5.0 * (1.0 - d * d)),
            0.1 * torch.exp(-10.0 * ((q[:, 2] - HEIGHT).abs() - DEAD).clamp(min=0.0)),
            0.15 * torch.exp(-2.0 * ((q[:, 7:17] - u[:, IN_POSE: IN_POSE + 10]) ** 2).sum(1)),
            -1e-4 * (v[:, 6:32] ** 2).sum(1),
            -0.01 * ((u[:, IN_ACT: IN_ACT + 10] - u[:, IN_PREV: IN_PREV + 10]) ** 2).sum(1),
            -0.001 * u[:, IN_ACT: IN_ACT + 10].abs().sum(1),
            0.05 * torch.exp(-(v[:, 12:15] ** 2).sum(1).sqrt()) * u[:, IN_CLOCK],
            0.05 * torch.exp(-(v[:, 25:28] ** 2).sum(1).sqrt()) * u[:, IN_CLOCK + 1],
            0.05 / (1.0 + 0.1 * s[:, IMU_GYRO: IMU_GYRO + 3].abs().amax(1)),
            -0.02 * grav.abs().sum(1)], dim=1)
        r = terms.sum(1).clamp(LO, HI)
        self.rows[e0: e0 + cnt] = terms.float()
        self.rew[e0: e0 + cnt] = r.float()
        ended = self.done[e0: e0 + cnt] != 0
        ret = self.ret[e0: e0 + cnt]
        self.fin[e0: e0 + cnt] = torch.where(ended, ret, self.fin[e0: e0 + cnt])
        self.ret[e0: e0 + cnt] = torch.where(ended, torch.zeros_like(ret), ret) + r

    def launch(self):
        b, p = self.b, self.policy_step
        self.policy_step += 1
        for (first, cnt), st in zip(self.ranges, self.streams):
            r0, k = bench.rows_of_group_in_range(bench.restart_group(p), 0, first, cnt)
            if k:
                b.reset_envs(r0, bench.NGROUP, k, self.init_row.data_ptr(), self.init_row.data_ptr() + 8 * self.pod.nq, st.cuda_stream)
            b.step_range(first, cnt, NSUB, st.cuda_stream)
            if self.leg == "reward":
                b.reward(first, cnt, reset_ptr=self.done.data_ptr() + 4 * first, stream=st.cuda_stream)
            elif self.leg == "torch":
                with torch.cuda.stream(st):
                    self.torch_reward(first, cnt)

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
            rew = self.rew.cpu().numpy()
            out["reward"] = {"terms": self.nterms, "dtype": "float32", "term_rows": True, "returns": True}
            out["finite_rewards"] = int(np.isfinite(rew).sum())
            out["reward_mean"], out["reward_min"], out["reward_max"] = float(rew.mean()), float(rew.min()), float(rew.max())
        if self.leg == "reward":
            out["reward_launches"] = self.b.reward_launches()
            # the call alone over the whole batch on an idle device: device events round 20 calls
            ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            st = self.streams[0]
            self.b.reward(0, self.n, stream=st.cuda_stream)
            torch.cuda.synchronize()
            with torch.cuda.stream(st):
                ev0.record()
                for _ in range(20):
                    self.b.reward(0, self.n, stream=st.cuda_stream)
                ev1.record()
            torch.cuda.synchronize()
            out["reward_call_alone_us"] = 1000.0 * ev0.elapsed_time(ev1) / 20
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
    out = {"tool": "reward_rate", "model": "cassie", "envs": a.envs, "substeps_per_launch": NSUB, "launches_per_region": a.launches,
           "warmup_launches": a.warmup, "regions_per_leg": a.repeats,
           "mode": "CM_DRIVE_PD_SAFE, 50 fused substeps per launch, two env ranges on two streams, restarts on the benchmark's schedule (config 2); "
                   "the legs alternate region by region in one process; a reward per range behind its step launch",
           "yardstick": "loop"}
    if a.parent_lib:
        # (first, in processes of their own: one library per process; this process has not touched the GPU yet)
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
    if "reward" in out and "torch" in out:
        one, many = out["reward"]["env_steps_per_s_median"], out["torch"]["env_steps_per_s_median"]
        spread = max(out[name]["spread_percent_of_median"] for name in LEGS if name in out)
        out["cheaper_reward_leg"] = "reward" if one > many else "torch"
        out["difference_of_the_reward_legs_percent_of_loop"] = 100.0 * abs(one - many) / out["loop"]["env_steps_per_s_median"] if "loop" in out else None
        out["largest_spread_of_a_leg_percent"] = spread
        if out["difference_of_the_reward_legs_percent_of_loop"] is not None:
            out["difference_over_spread"] = out["difference_of_the_reward_legs_percent_of_loop"] / spread
    if "parent_loop" in out:
        par, own = out["parent_loop"], out["loop_alone"]
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
