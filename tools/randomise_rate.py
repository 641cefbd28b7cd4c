#!/usr/bin/env python3
"""Env-steps per second of 4096 cassie.xml envs in config 2's mode -- CM_DRIVE_PD_SAFE, 50 fused substeps per launch, the batch
as two env ranges on two streams -- in three settings: nothing randomised; the five parameters of
phys_batch_randomize that existed first (masses, inertial offsets, inertias, damping, friction) + set_const; all nine, with
every env's own stair box under the feet, floor tilt and spring stiffness (the step kernel then reads geometry and springs from
the env's block).  Prints one JSON line.  Needs a GPU.

    python tools/randomise_rate.py [--envs 4096] [--launches 40] [--warmup 5] [--repeats 3]
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
import geometry_randomise_check as gc  # noqa: E402
import randomise_check as rc  # noqa: E402

NSUB = 50


def settings(pod, model, n):
    five = gc.own_params(pod, n)
    five.update(rc.random_params(model, n, seed=3))
    rng = np.random.default_rng(5)
    nine = dict(five)
    gp = five["geom_pos"].reshape(n, pod.ngeom, 3).copy()
    gq = five["geom_quat"].reshape(n, pod.ngeom, 4).copy()
    box = 1 + np.arange(n) % 15
    gp[np.arange(n), box] = np.stack([rng.uniform(-0.3, 0.3, n), rng.uniform(-0.3, 0.3, n), rng.uniform(-1.03, -0.97, n)], 1)
    ang = np.radians(rng.uniform(0, 3, n)) / 2
    phi = rng.uniform(0, 2 * np.pi, n)
    gq[:, 0] = np.stack([np.cos(ang), np.sin(ang) * np.cos(phi), np.sin(ang) * np.sin(phi), np.zeros(n)], 1)
    nine["geom_pos"], nine["geom_quat"] = gp.reshape(n, -1), gq.reshape(n, -1)
    nine["jnt_stiffness"] = five["jnt_stiffness"] * rng.uniform(0.8, 1.2, five["jnt_stiffness"].shape)
    return {"unrandomised": None, "five_fields": (five, tuple(rc.PARAM_IDS)), "all_nine_stairs": (nine, tuple(gc.ALL_IDS))}


def rate(model, n, what, launches, warmup):
    b = Batch(model, n)
    try:
        if what is not None:
            params, fields = what
            for f in fields:
                b.randomize(gc.ALL_IDS[f], params[f])
            b.set_const()
        b.set(P.F_QPOS, np.tile(model.qpos_init(), (n, 1)))
        b.forward()
        b.set(P.F_PD_KP, np.tile(bench.PD_KP, (n, 1)))
        b.set(P.F_PD_KD, np.tile(bench.PD_KD, (n, 1)))
        b.set(P.F_PD_PTARGET, bench.PD_OFFSET + np.random.default_rng(1).uniform(-0.3, 0.3, (n, 10)))
        b.set_drive_mode(P.DRIVE_PD_SAFE)
        b.sync()
        streams, half = [torch.cuda.Stream(), torch.cuda.Stream()], n // 2

        def launch():
            for k, st in enumerate(streams):
                b.step_range(k * half, n - half if k else half, NSUB, st.cuda_stream)
        for _ in range(warmup):
            launch()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(launches):
            launch()
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        w, info = b.warnings()
        return n * NSUB * launches / dt, int(w.astype(bool).sum()), float(info[:, 0].mean())
    finally:
        b.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--launches", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=3)
    a = ap.parse_args()
    model = Model("cassie")
    out = {"tool": "randomise_rate", "model": "cassie", "envs": a.envs, "substeps_per_launch": NSUB, "launches": a.launches,
           "mode": "CM_DRIVE_PD_SAFE, 50 fused substeps per launch, two env ranges on two streams (config 2)", "repeats": a.repeats}
    for name, what in settings(model.pod, model, a.envs).items():
        runs = [rate(model, a.envs, what, a.launches, a.warmup) for _ in range(a.repeats)]
        out[name] = {"env_steps_per_s_median": float(np.median([r[0] for r in runs])), "runs": [r[0] for r in runs],
                     "envs_with_warnings": runs[-1][1], "mean_contacts_last_step": runs[-1][2]}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
