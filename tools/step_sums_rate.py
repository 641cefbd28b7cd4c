#!/usr/bin/env python3
"""What the step sums (Batch.enable_step_sums) cost config 2's loop: env-steps per second of 4096 envs in CM_DRIVE_PD_SAFE, 50 fused
substeps per launch, the batch as two env ranges on two streams -- with the sums off and on, the two legs ALTERNATING in one process on
one batch each (other people's work shares the host: a difference is read against the spread of the same leg's repeats), for cassie
and cassie_hfield.  The "off" leg is the loop of tools/randomise_rate.py's "unrandomised" setting: its rate is what the commit before
the step sums measures for that loop.  Writes one JSON object to --out (default profiles/step_sums_rate.json) and prints it.  Needs a GPU.

    python tools/step_sums_rate.py [--envs 4096] [--launches 40] [--warmup 5] [--repeats 5] [--models cassie cassie_hfield] [--out FILE]
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
import golden_physics as G  # noqa: E402
from cassie_amd import Batch, Model  # noqa: E402
from cassie_amd import phys as P  # noqa: E402

NSUB = 50


def make(model, n, sums):
    b = Batch(model, n)
    q = np.tile(model.qpos_init(), (n, 1))
    hf = G.terrain(model.name)
    if hf is not None:
        b.set_hfield(hf)
        for e in range(n):
            q[e, 0], q[e, 1] = G.start_xy(model.name, e)
    b.set(P.F_QPOS, q)
    b.forward()
    b.set(P.F_PD_KP, np.tile(bench.PD_KP, (n, 1)))
    b.set(P.F_PD_KD, np.tile(bench.PD_KD, (n, 1)))
    b.set(P.F_PD_PTARGET, bench.PD_OFFSET + np.random.default_rng(1).uniform(-0.3, 0.3, (n, 10)))
    b.set_drive_mode(P.DRIVE_PD_SAFE)
    if sums:
        b.enable_step_sums()
    b.sync()
    return b


def window(b, n, streams, launches):
    """launches x (two ranges on two streams) -> env-steps per second, by the host clock around work that ends in a device synchronise."""
    half = n // 2
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(launches):
        for k, st in enumerate(streams):
            b.step_range(k * half, n - half if k else half, NSUB, st.cuda_stream)
    torch.cuda.synchronize()
    return n * NSUB * launches / (time.perf_counter() - t0)


def measure(name, n, launches, warmup, repeats, which):
    model = Model(name)
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    legs = {leg: make(model, n, leg == "on") for leg in which}
    try:
        for b in legs.values():
            window(b, n, streams, warmup)
        runs = {leg: [] for leg in legs}
        for _ in range(repeats):            # off, on, off, on ...: both legs see the same drift of the box
            for leg, b in legs.items():
                runs[leg].append(window(b, n, streams, launches))
        out = {}
        for leg, b in legs.items():
            w, info = b.warnings()
            r = np.array(runs[leg])
            out[leg] = {"env_steps_per_s_median": float(np.median(r)), "runs": [float(v) for v in r],
                        "spread_rel": float((r.max() - r.min()) / np.median(r)), "envs_with_warnings": int(w.astype(bool).sum()),
                        "mean_contacts_last_step": float(info[:, 0].mean())}
        if "on" in legs:
            s = legs["on"].step_sums()
            out["on"]["count_of_the_last_launch"] = [float(s["count"].min()), float(s["count"].max())]
        if len(legs) == 2:
            out["cost_rel"] = 1.0 - out["on"]["env_steps_per_s_median"] / out["off"]["env_steps_per_s_median"]
            # ... and pair by pair: an "on" window against the "off" window right in front of it sees the box in the same state
            pairs = 1.0 - np.array(runs["on"]) / np.array(runs["off"])
            out["cost_rel_pairs"] = [float(v) for v in pairs]
            out["cost_rel_pairs_median"] = float(np.median(pairs))
        return out
    finally:
        for b in legs.values():
            b.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--launches", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--models", nargs="+", default=["cassie", "cassie_hfield"])
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "step_sums_rate.json"))
    ap.add_argument("--legs", nargs="+", default=["off", "on"], choices=["off", "on"],
                    help="'off' alone also runs on a library built from the commit before the step sums (CASSIE_LIB)")
    a = ap.parse_args()
    out = {"tool": "step_sums_rate", "envs": a.envs, "substeps_per_launch": NSUB, "launches": a.launches, "repeats": a.repeats,
           "mode": "CM_DRIVE_PD_SAFE, 50 fused substeps per launch, two env ranges on two streams (config 2); legs alternate in one process"}
    for name in a.models:
        out[name] = measure(name, a.envs, a.launches, a.warmup, a.repeats, a.legs)
    text = json.dumps(out)
    with open(a.out, "w") as f:
        f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
