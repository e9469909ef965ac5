"""Frames per second with a geometry update before every frame (fr_update_geometry_enqueue against the synchronous
fr_update_geometry): the bench workload (bunny 4K, 4 spp, GI 3, signed log-polar mask), positions in device
memory, a refit + normal recompute before every untimed fr_frame. Four arms, one context each (so the synchronous
arm runs exactly the path it ran before enqueued updates existed), all in one process:
  S  fr_update_geometry(device, FR_BVH_REFIT, FR_NORMALS_RECOMPUTE), then fr_frame
  E  fr_update_geometry_enqueue(FR_NORMALS_RECOMPUTE), fr_frame, fr_geometry_consumed on the producer's stream
  D  E on a context with fr_set_geometry_overlap on (the update beside the previous frame's path trace)
  0  fr_frame alone (no update)
The arms alternate, six rounds, the order swapped after three; a round of an arm is 30 warm-up frames and 60 timed
ones (host clock around the loop, the context synchronised before and after). Throughput mode, then latency mode.
Any failing call ends the script.

Writes one JSON line per (mode, arm, round) to --out (default profiles/update_enqueue_probe.jsonl) and prints a
markdown table. Usage: update_enqueue_probe.py [--out FILE] [--width W --height H] [--arms S,E,D,0] [--modes
throughput,latency] [--rounds N] (the last three narrow a run down for a profiler: one arm alone, one mode)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, os.path.join(ROOT, "foveated-rendering-using-ray-tracing_amd"))
import torch  # noqa: E402  before libfovrt: one HIP runtime in the process (the positions live in tensors)
import fovrt  # noqa: E402

ASSET_FILES = ("CedarCity.hdr", "grid.ppm", "bunny/bunny.PPM", "vokselia_spawn/vokselia_spawn.png")
WARMUP, TIMED, ROUNDS = 30, 60, 6
ARMS = ("S", "E", "D", "0")


def run(t, arm, dev, n, frames, stream):
    for i in range(frames):
        if arm == "S":
            t.set_positions_device(dev[i & 1].data_ptr(), n, update="refit", normals="recompute")
        elif arm in ("E", "D"):
            t.update_geometry_enqueue(dev[i & 1], ntris=n, normals="recompute")
        t.frame(timing=False)
        if arm in ("E", "D"):
            t.geometry_consumed(stream)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "update_enqueue_probe.jsonl"))
    ap.add_argument("--width", type=int, default=3840)
    ap.add_argument("--height", type=int, default=2160)
    ap.add_argument("--arms", default=",".join(ARMS))
    ap.add_argument("--modes", default="throughput,latency")
    ap.add_argument("--rounds", type=int, default=ROUNDS)
    args = ap.parse_args()
    W, H = args.width, args.height
    arms, modes, rounds = tuple(args.arms.split(",")), tuple(args.modes.split(",")), args.rounds
    assert set(arms) <= set(ARMS) and set(modes) <= {"throughput", "latency"} and rounds >= 1
    have = all(os.path.exists(os.path.join(fovrt.DEFAULT_ASSET_DIR, p)) for p in ASSET_FILES)
    rows = []
    for mode in modes:
        ctx = {}
        for arm in arms:
            t = fovrt.PathTracer(fovrt.Config(width=W, height=H, scene=fovrt.SCENE_BUNNY,
                                              mask_mode=fovrt.MASK_LOGPOLAR_SIGNED, spp=4, diffuse_max_depth=3,
                                              texture_mode=0 if have else 1))
            t.initialize()
            t.update_optix_variables(fovrt.Camera.preset(fovrt.SCENE_BUNNY, W, H))
            if mode == "latency":
                t.set_pipeline_mode(fovrt.PIPELINE_LATENCY)
            if arm == "D":
                t.set_geometry_overlap(True)
            ctx[arm] = t
        base = ctx[arms[0]].scene_arrays()["pos"].reshape(-1, 3, 3).copy()
        n = base.shape[0]
        dev = []
        for phase in (0.0, 1.0):  # two poses of one wave: every update moves every vertex
            pos = base.copy()
            pos[..., 1] += np.float32(0.05) * np.sin(np.float32(3.0) * base[..., 0] + np.float32(phase)).astype(np.float32)
            dev.append(torch.from_numpy(pos.reshape(-1, 9)).to("cuda:0"))
        torch.cuda.synchronize()
        stream = torch.cuda.current_stream()
        for r in range(rounds):
            order = arms if r < (rounds + 1) // 2 else arms[::-1]
            for arm in order:
                t = ctx[arm]
                run(t, arm, dev, n, WARMUP, stream)
                t.synchronize()
                t0 = time.perf_counter()
                run(t, arm, dev, n, TIMED, stream)
                t.synchronize()
                dt = time.perf_counter() - t0
                row = dict(mode=mode, arm=arm, round=r, width=W, height=H, tris=n, frames=TIMED, fps=TIMED / dt,
                           ms_per_frame=1e3 * dt / TIMED)
                print(json.dumps(row), flush=True)
                rows.append(row)
        for arm in set(arms) & {"E", "D"}:
            applied, rejected = ctx[arm].geometry_update_status()
            assert (applied, rejected) == (rounds * (WARMUP + TIMED), 0), (arm, applied, rejected)
        torch.cuda.synchronize()
        for t in ctx.values():
            t.destroy()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        for row in rows:
            f.write(json.dumps(row) + "\n")
    print("\n| mode | arm | fps per round | median | min | max | spread (max - min) |")
    print("|---|---|---|---|---|---|---|")
    for mode in modes:
        for arm in arms:
            v = [row["fps"] for row in rows if row["mode"] == mode and row["arm"] == arm]
            print(f"| {mode} | {arm} | {' '.join(f'{x:.1f}' for x in v)} | {float(np.median(v)):.1f} | {min(v):.1f} | "
                  f"{max(v):.1f} | {max(v) - min(v):.1f} |")


if __name__ == "__main__":
    main()
