#!/usr/bin/env python3
"""What the action path per policy step costs config 2's loop -- 4096 cassie.xml envs, CM_DRIVE_PD_SAFE, 50 fused substeps per launch, the
batch as two env ranges on two streams with nothing joining them, restarts on bench.py's schedule -- in three legs that ALTERNATE in one
process on one box, fenced timed regions, ten each:

  loop          the loop alone, with the targets of every policy step bound as the benchmark binds them: the four target tensors the
                action path settles into (the actions repeat every four policy steps, and the filter forgets its start), made on the
                host once.  THE YARDSTICK.
  act           the same plus one phys_batch_act per range and policy step, on the range's stream IN FRONT of its step launch: ten
                columns from a float32 action tensor into F_PD_PTARGET on a reference pose from the caller's input, clipped to [-1, 1], a
                delay line of depth 2 with per-env delays, a low-pass of 0.5, the clip of the target, and the action rows (float32).
  torch         the same action path written with torch operations on the same streams: the clip, a ring buffer of the last three actions
                with a per-env gather, the filter, the affine map, the clip, the cast, the copy into the bound target tensor and the
                previous-action bookkeeping.  What a user does today.

In every leg F_PD_PTARGET is bound to a torch tensor and the robots are driven by the same targets (to float32 rounding), so the legs
differ in what precedes a step launch alone, not in what the step kernel meets.  The two action legs are given the same actions, pose and
delays: their targets at the end are compared (the torch leg filters in float32).

--parent-lib PATH runs the `loop` leg alone in child processes, in the order parent, this build, this build, parent, against another
build of the library (the parent commit's) and against this one: like against like, one batch in a fresh process of its own, the regions
of a build's two runs pooled.  No stepping kernel changes with the action rows, so this build's median should lie inside the parent's
regions.

Also times the act call alone over the whole batch on an idle device.  Every region is recorded.  Prints one JSON line; `--out` also
writes it to a file.  Needs a GPU.

    python tools/action_rate.py [--envs 4096] [--launches 20] [--warmup 10] [--repeats 10] [--only NAME] [--out profiles/action_rate.json]
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
LEGS = ("loop", "act", "torch")
NACT, DELAY_MAX, SMOOTH, SCALE, OUT_HALF = 10, 2, 0.5, 0.3, 0.6
# the input's columns: the reference pose of ten joints | two clock coefficients
IN_POSE, NINPUT = 0, 12


def act_columns():
    return [P.act_col(P.F_PD_PTARGET, j, lo=-1.0, hi=1.0, smooth=SMOOTH, bfield=P.ACT_INPUT, bindex=IN_POSE + j, scale=SCALE,
                      out_lo=float(bench.PD_OFFSET[j]) - OUT_HALF, out_hi=float(bench.PD_OFFSET[j]) + OUT_HALF) for j in range(NACT)]


class Leg:
    """One batch running config 2's loop, with what its leg adds in front of every range's step launch."""

    def __init__(self, model, n, leg):
        pod = model.pod
        self.leg, self.n, self.pod = leg, n, pod
        self.b = b = Batch(model, n)
        dev = torch.device("cuda")
        rng = np.random.default_rng(1)
        tgt0 = bench.PD_OFFSET + rng.uniform(-0.3, 0.3, (n, NACT))
        self.tgt = torch.from_numpy(tgt0).to(dev)
        torch.cuda.synchronize()
        b.bind(P.F_PD_PTARGET, self.tgt.data_ptr())
        b.set(P.F_QPOS, np.tile(model.qpos_init(), (n, 1)))
        b.forward()
        sens0 = b.get(P.F_SENSORDATA, 0, 1)[0]
        b.set(P.F_PD_KP, np.tile(bench.PD_KP, (n, 1)))
        b.set(P.F_PD_KD, np.tile(bench.PD_KD, (n, 1)))
        b.set_drive_mode(P.DRIVE_PD_SAFE)
        self.init_row = torch.from_numpy(np.concatenate([model.qpos_init(), sens0])).cuda()
        # what a policy and its caller hand the action path: the actions, the pose and the clock, the per-env latency
        self.actions = torch.from_numpy(rng.uniform(-1.5, 1.5, (4, n, NACT)).astype(np.float32)).to(dev)
        inp = np.zeros((n, NINPUT), dtype=np.float32)
        inp[:, IN_POSE: IN_POSE + NACT] = bench.PD_OFFSET + rng.uniform(-0.1, 0.1, (n, NACT))
        self.inp = torch.from_numpy(inp).to(dev)
        delay = rng.integers(0, DELAY_MAX + 1, n).astype(np.int32)
        self.delay = torch.from_numpy(delay).to(dev)
        if leg == "loop":
            # the path on the host, 64 policy steps (the filter's start has decayed below an ulp), then the four steps of a cycle
            u = np.clip(self.actions.cpu().numpy().astype(np.float64), -1.0, 1.0)
            pose, y, cycle, envs = inp[:, IN_POSE: IN_POSE + NACT].astype(np.float64), None, [], np.arange(n)
            for p in range(68):
                z = u[np.maximum(p - delay, 0) % 4, envs]
                y = z if y is None else y + SMOOTH * (z - y)
                if p >= 64:
                    cycle.append(np.clip(pose + SCALE * y, bench.PD_OFFSET - OUT_HALF, bench.PD_OFFSET + OUT_HALF))
            self.cycle = torch.from_numpy(np.array(cycle)).to(dev)
        if leg == "act":
            b.configure_actions(act_columns(), delay_max=DELAY_MAX, dtype=np.float32, seed=1)
            b.bind_action_input(self.inp.data_ptr(), NINPUT, NINPUT, torch.float32)
            b.bind_action_delay(self.delay.data_ptr())
        if leg == "torch":
            self.ring = torch.zeros((DELAY_MAX + 1, n, NACT), dtype=torch.float32, device=dev)
            self.filt = torch.zeros((n, NACT), dtype=torch.float32, device=dev)
            self.now = torch.zeros((n, NACT), dtype=torch.float32, device=dev)
            self.prev = torch.zeros((n, NACT), dtype=torch.float32, device=dev)
            self.envs = torch.arange(n, device=dev)
            self.delay64 = self.delay.long()
            off = torch.from_numpy(np.asarray(bench.PD_OFFSET, dtype=np.float64)).to(dev)
            self.out_lo, self.out_hi = off - OUT_HALF, off + OUT_HALF
            self.first = True
        b.sync()
        torch.cuda.synchronize()
        self.streams, half = [torch.cuda.Stream(), torch.cuda.Stream()], n // 2
        self.ranges = [(0, half), (half, n - half)]
        self.policy_step = 0
        self.rates = []

    def torch_actions(self, e0, cnt, p):
        """The targets of the range as a user makes them today (on the current stream)."""
        s = slice(e0, e0 + cnt)
        u = self.actions[p % 4, s].clamp(-1.0, 1.0)
        head = p % (DELAY_MAX + 1)
        if self.first:
            self.ring[:, s] = u
            y = u
        else:
            self.ring[head, s] = u
            slot = (head - self.delay64[s]) % (DELAY_MAX + 1)
            z = self.ring[slot, self.envs[s]]
            f = self.filt[s]
            y = f + SMOOTH * (z - f)
        self.filt[s] = y
        t = (self.inp[s, IN_POSE: IN_POSE + NACT].double() + SCALE * y.double())
        self.tgt[s] = torch.minimum(torch.maximum(t, self.out_lo), self.out_hi)
        self.prev[s] = u if self.first else self.now[s]
        self.now[s] = u

    def launch(self):
        b, p = self.b, self.policy_step
        self.policy_step += 1
        if self.leg == "act":
            b.bind_actions(self.actions[p % 4].data_ptr(), NACT, torch.float32)
        elif self.leg == "loop":
            b.bind(P.F_PD_PTARGET, self.cycle[p % 4].data_ptr())
        for (first, cnt), st in zip(self.ranges, self.streams):
            r0, k = bench.rows_of_group_in_range(bench.restart_group(p), 0, first, cnt)
            if k:
                b.reset_envs(r0, bench.NGROUP, k, self.init_row.data_ptr(), self.init_row.data_ptr() + 8 * self.pod.nq, st.cuda_stream)
            if self.leg == "act":
                b.act(first, cnt, stream=st.cuda_stream)
            elif self.leg == "torch":
                with torch.cuda.stream(st):
                    self.torch_actions(first, cnt, p)
            b.step_range(first, cnt, NSUB, st.cuda_stream)
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
            self.targets = self.tgt.cpu().numpy()
            out["columns"] = NACT
            out["finite_target_rows"] = int(np.isfinite(self.targets).all(axis=1).sum())
        if self.leg == "act":
            rows = self.b.action_rows()
            out["act_launches"] = self.b.action_launches()
            out["row"] = {"columns": NACT, "frames": 3, "dtype": "float32", "bytes_per_env": 4 * 3 * NACT, "state_bytes_per_env": 8 * (DELAY_MAX + 3) * NACT}
            out["rows_whose_now_and_prev_differ"] = int((rows[:, P.ACT_NOW] != rows[:, P.ACT_PREV]).any(axis=1).sum())
            out["rows_whose_applied_and_now_differ"] = int((rows[:, P.ACT_APPLIED] != rows[:, P.ACT_NOW]).any(axis=1).sum())
            # the call alone over the whole batch on an idle device: device events round 20 calls
            ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            st = self.streams[0]
            self.b.act(0, self.n, stream=st.cuda_stream)
            torch.cuda.synchronize()
            with torch.cuda.stream(st):
                ev0.record()
                for _ in range(20):
                    self.b.act(0, self.n, stream=st.cuda_stream)
                ev1.record()
            torch.cuda.synchronize()
            out["act_call_alone_us"] = 1000.0 * ev0.elapsed_time(ev1) / 20
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
    out = {"tool": "action_rate", "model": "cassie", "envs": a.envs, "substeps_per_launch": NSUB, "launches_per_region": a.launches,
           "warmup_launches": a.warmup, "regions_per_leg": a.repeats,
           "mode": "CM_DRIVE_PD_SAFE, 50 fused substeps per launch, two env ranges on two streams, restarts on the benchmark's schedule (config 2); "
                   "the legs alternate region by region in one process; the action path of a range in front of its step launch",
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
        by = {leg.leg: leg for leg in legs}
        if "act" in by and "torch" in by:
            # (the same actions, pose and delays through the same number of policy steps; read before the act leg's timing calls)
            out["targets_largest_difference_act_against_torch"] = float(np.abs(by["act"].targets - by["torch"].targets).max())
    finally:
        for leg in legs:
            leg.close()
    if "loop" in out:
        base = out["loop"]["env_steps_per_s_median"]
        for name in LEGS[1:]:
            if name in out:
                out[name]["cost_of_the_loop_percent"] = 100.0 * (1.0 - out[name]["env_steps_per_s_median"] / base)
        out["loop_spread_percent"] = out["loop"]["spread_percent_of_median"]
    if "act" in out and "torch" in out:
        one, many = out["act"]["env_steps_per_s_median"], out["torch"]["env_steps_per_s_median"]
        out["cheaper_action_leg"] = "act" if one > many else "torch"
        out["act_loses_less_than_torch"] = bool(one > many)
        out["largest_spread_of_a_leg_percent"] = max(out[name]["spread_percent_of_median"] for name in LEGS if name in out)
        if "loop" in out:
            out["difference_of_the_action_legs_percent_of_loop"] = 100.0 * abs(one - many) / out["loop"]["env_steps_per_s_median"]
            out["difference_over_spread"] = out["difference_of_the_action_legs_percent_of_loop"] / out["largest_spread_of_a_leg_percent"]
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
