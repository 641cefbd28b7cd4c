#!/usr/bin/env python3
"""What ending and restarting episodes on the device costs config 2's loop -- 4096 cassie.xml envs, CM_DRIVE_PD_SAFE, 50 fused
substeps per launch, the batch as two env ranges on two streams -- in three settings, one process, fenced timed regions:

  reset_envs     the loop as it was: phys_batch_reset_envs on bench.py's schedule (env e restarts from the init pose every
                 bench.NGROUP policy steps at phase e % NGROUP).  THE YARDSTICK.
  time_limit     phys_batch_end_episodes per range per policy step with only max_steps = NGROUP set and the step counters started
                 at e % NGROUP: the same number of envs restart per policy step.
  all_rules      the same with every rule on (height, tilt, WARN_DIVERGED, non-finite).

Prints one JSON line with the regions of each setting (env-steps per second).  Needs a GPU.

    python tools/episode_rate.py [--envs 4096] [--launches 40] [--warmup 20] [--repeats 5]
"""
import argparse
import json
import os
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
SETTINGS = {"reset_envs": None,
            "time_limit": dict(max_steps=bench.NGROUP),
            "all_rules": dict(max_steps=bench.NGROUP, min_height=0.4, min_upright=0.3, warn_mask=P.WARN_DIVERGED, nonfinite=True)}


def regions(model, n, rules, launches, warmup, repeats):
    pod = model.pod
    b = Batch(model, n)
    try:
        q0 = model.qpos_init()
        b.set(P.F_QPOS, np.tile(q0, (n, 1)))
        b.forward()
        sens0 = b.get(P.F_SENSORDATA, 0, 1)[0]
        b.set(P.F_PD_KP, np.tile(bench.PD_KP, (n, 1)))
        b.set(P.F_PD_KD, np.tile(bench.PD_KD, (n, 1)))
        b.set(P.F_PD_PTARGET, bench.PD_OFFSET + np.random.default_rng(1).uniform(-0.3, 0.3, (n, 10)))
        b.set_drive_mode(P.DRIVE_PD_SAFE)
        init_row = torch.from_numpy(np.concatenate([q0, sens0])).cuda()
        steps0 = None
        if rules is not None:
            b.enable_episodes(**rules)
            b.set_reset_bank(b.make_reset_bank(q0[None]))
            steps0 = torch.from_numpy((np.arange(n) % bench.NGROUP).astype(np.int32)).cuda()
            b.bind_episode(P.EP_STEPS, steps0.data_ptr())
        b.sync()
        torch.cuda.synchronize()
        streams, half = [torch.cuda.Stream(), torch.cuda.Stream()], n // 2
        ranges = [(0, half), (half, n - half)]
        policy_step = [0]

        def launch():
            p = policy_step[0]
            policy_step[0] += 1
            for (first, cnt), st in zip(ranges, streams):
                if rules is None:
                    r0, k = bench.rows_of_group_in_range(bench.restart_group(p), 0, first, cnt)
                    if k:
                        b.reset_envs(r0, bench.NGROUP, k, init_row.data_ptr(), init_row.data_ptr() + 8 * pod.nq, st.cuda_stream)
                b.step_range(first, cnt, NSUB, st.cuda_stream)
                if rules is not None:
                    b.end_episodes(first, cnt, True, stream=st.cuda_stream)
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
        info = {"env_steps_per_s_median": float(np.median(out)), "regions": out, "envs_with_warnings": int(b.warnings()[0].astype(bool).sum())}
        if rules is not None:
            done, reason, steps, count, _ = b.episodes()
            info["episodes_ended"] = int(count.sum())
            info["ended_in_last_step_by_reason_bit"] = {str(bit): int(((reason & bit) != 0).sum()) for bit in (1, 2, 4, 8, 16, 32)}
        return info
    finally:
        b.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--launches", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--only", choices=sorted(SETTINGS), default=None, help="one setting only (e.g. under a kernel trace)")
    a = ap.parse_args()
    model = Model("cassie")
    out = {"tool": "episode_rate", "model": "cassie", "envs": a.envs, "substeps_per_launch": NSUB, "launches_per_region": a.launches,
           "warmup_launches": a.warmup, "mode": "CM_DRIVE_PD_SAFE, 50 fused substeps per launch, two env ranges on two streams (config 2)",
           "yardstick": "reset_envs"}
    for name, rules in SETTINGS.items():
        if a.only in (None, name):
            out[name] = regions(model, a.envs, rules, a.launches, a.warmup, a.repeats)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
