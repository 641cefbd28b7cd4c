#!/usr/bin/env python3
"""What saving and forking envs through the bank of full states (Batch.save_states / restore_states) costs config 2's loop: env-steps
per second of 4096 envs in CM_DRIVE_PD_SAFE, 50 fused substeps per launch, the batch as two env ranges on two streams, nothing joining
them and no host read -- three legs ALTERNATING in one process on one batch each (other people's work shares the host: a difference is
read against the spread of the same leg's windows):

    loop   the loop as it is
    save   ... plus one save of every env of the range behind every step launch (slot = env)
    fork   ... plus a save and a fan-out restore: every env of a group of --fan envs takes the slot of the group's first env
           (device slots, set up before the windows)

With --parent-lib the "loop" leg is also run, in a child process before and after the legs, on a library built from the commit before
the bank (CASSIE_LIB): the two must agree within the leg's own window spread.  Writes one JSON object to --out (default
profiles/state_rate.json) and prints it.  Needs a GPU.

    python tools/state_rate.py [--envs 4096] [--launches 40] [--warmup 5] [--repeats 5] [--fan 16] [--parent-lib FILE] [--out FILE]
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

NSUB = 50
LEGS = ("loop", "save", "fork")


def make(model, n, leg, fan):
    """(The envs of a fan-out group share their targets, in every leg: a forked env then is where its own run would have been, and the
    three legs step the same physics -- a fork into envs with other targets would measure the falls it causes, not the copy.)"""
    import bench
    from cassie_amd import Batch
    from cassie_amd import phys as P
    b = Batch(model, n)
    b.set(P.F_QPOS, np.tile(model.qpos_init(), (n, 1)))
    b.forward()
    b.set(P.F_PD_KP, np.tile(bench.PD_KP, (n, 1)))
    b.set(P.F_PD_KD, np.tile(bench.PD_KD, (n, 1)))
    b.set(P.F_PD_PTARGET, np.repeat(bench.PD_OFFSET + np.random.default_rng(1).uniform(-0.3, 0.3, (n // fan, 10)), fan, axis=0))
    b.set_drive_mode(P.DRIVE_PD_SAFE)
    if leg != "loop":
        b.configure_states(n)
    b.sync()
    return b


def window(b, n, streams, launches, leg, take_ptr):
    """launches x (two ranges on two streams) -> env-steps per second, by the host clock around work that ends in a device synchronise."""
    import torch
    half = n // 2
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(launches):
        for k, st in enumerate(streams):
            e0, cnt = k * half, n - half if k else half
            b.step_range(e0, cnt, NSUB, st.cuda_stream)
            if leg != "loop":
                b.save_states(env0=e0, n=cnt, stream=st.cuda_stream)
            if leg == "fork":
                b.restore_states(env0=e0, n=cnt, slots_ptr=take_ptr + 4 * e0, stream=st.cuda_stream)
    torch.cuda.synchronize()
    return n * NSUB * launches / (time.perf_counter() - t0)


def measure(n, launches, warmup, repeats, which, fan):
    import torch
    from cassie_amd import Model
    model = Model("cassie")
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    take = torch.from_numpy((np.arange(n) // fan * fan).astype(np.int32)).cuda()      # (a group never straddles the two ranges: fan divides n / 2)
    assert (n // 2) % fan == 0
    legs = {leg: make(model, n, leg, fan) for leg in which}
    try:
        for leg, b in legs.items():
            window(b, n, streams, warmup, leg, take.data_ptr())
        runs = {leg: [] for leg in legs}
        for _ in range(repeats):            # loop, save, fork, loop ...: every leg sees the same drift of the box
            for leg, b in legs.items():
                runs[leg].append(window(b, n, streams, launches, leg, take.data_ptr()))
        out = {}
        for leg, b in legs.items():
            w, _ = b.warnings()
            r = np.array(runs[leg])
            out[leg] = {"env_steps_per_s_median": float(np.median(r)), "windows": [float(v) for v in r],
                        "spread_rel": float((r.max() - r.min()) / np.median(r)), "envs_with_warnings": int(w.astype(bool).sum())}
            if leg != "loop":
                out[leg]["row_bytes"] = 8 * b.state_row_dim()
                out[leg]["bytes_per_call_and_range"] = 8 * b.state_row_dim() * (n // 2)
        for leg in legs:
            if leg != "loop" and "loop" in legs:
                out[leg]["cost_rel"] = 1.0 - out[leg]["env_steps_per_s_median"] / out["loop"]["env_steps_per_s_median"]
                pairs = 1.0 - np.array(runs[leg]) / np.array(runs["loop"])      # a window against the "loop" window right in front of it
                out[leg]["cost_rel_pairs_median"] = float(np.median(pairs))
        return out
    finally:
        for b in legs.values():
            b.close()


def parent_loop(a):
    """The "loop" leg on the parent commit's library, in a child process of its own."""
    env = dict(os.environ, CASSIE_LIB=os.path.abspath(a.parent_lib))
    cmd = [sys.executable, os.path.abspath(__file__), "--legs", "loop", "--envs", str(a.envs), "--launches", str(a.launches),
           "--warmup", str(a.warmup), "--repeats", str(a.repeats), "--fan", str(a.fan), "--out", "-"]
    text = subprocess.run(cmd, env=env, check=True, stdout=subprocess.PIPE, timeout=300).stdout.decode()
    return json.loads(text.strip().splitlines()[-1])["cassie"]["loop"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--launches", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--fan", type=int, default=16)
    ap.add_argument("--legs", nargs="+", default=list(LEGS), choices=LEGS)
    ap.add_argument("--parent-lib", default=None, help="libcassiemujoco.so built from the commit before the bank of full states")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "state_rate.json"), help="'-': print only")
    a = ap.parse_args()
    out = {"tool": "state_rate", "model": "cassie", "envs": a.envs, "substeps_per_launch": NSUB, "launches": a.launches, "repeats": a.repeats, "fan": a.fan,
           "mode": "CM_DRIVE_PD_SAFE, 50 fused substeps per launch, two env ranges on two streams (config 2); legs alternate in one process"}
    before = parent_loop(a) if a.parent_lib else None      # (ahead of this process's first use of the GPU)
    out["cassie"] = measure(a.envs, a.launches, a.warmup, a.repeats, a.legs, a.fan)
    if a.parent_lib:
        after = parent_loop(a)
        loop = out["cassie"]["loop"]
        both = before["windows"] + after["windows"]
        out["parent_commit_loop"] = {"before": before, "after": after, "env_steps_per_s_median": float(np.median(both))}
        out["loop_against_parent_rel"] = loop["env_steps_per_s_median"] / float(np.median(both)) - 1.0
        out["loop_agrees_with_parent_within_its_window_spread"] = bool(abs(out["loop_against_parent_rel"]) <= max(loop["spread_rel"], before["spread_rel"], after["spread_rel"]))
    text = json.dumps(out)
    if a.out != "-":
        with open(a.out, "w") as f:
            f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
