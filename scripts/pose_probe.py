"""Frames per second with a model pose before every frame (fr_set_model_transforms_enqueue) against the caller-array
form fed the same geometry (fr_update_geometry_enqueue) and against no update: the bench workload (bunny 4K, 4 spp,
GI 3, signed log-polar mask), the bunny turning about its vertical axis and the box sliding, a cycle of 8 poses.
Three arms, one context each, all in one process and on one build:
  P  fr_set_model_transforms_enqueue(m[i]), then fr_frame: 48 bytes per model from the host, no device memory
  E  fr_update_geometry_enqueue(X[i], N[i], FR_NORMALS_GIVEN), fr_frame, fr_geometry_consumed: the arrays pose_np
     gives for m[i], precomputed and uploaded before the loop
  0  fr_frame alone (no update)
The arms alternate, six rounds, the order swapped after three; a round of an arm is 30 warm-up frames and 60 timed
ones (host clock around the loop, the context synchronised before and after). Throughput mode, then latency mode.
Before the rounds the script checks that arms P and E hold the same positions and normals, byte for byte. Any failing
call ends the script.

--trace-frames N runs arm P alone for N frames and exits: the run to put under
`rocprofv3 --kernel-trace --stats -- python scripts/pose_probe.py --trace-frames 40` for k_pose's own time.

Writes one JSON line per (mode, arm, round) to --out (default profiles/pose_probe.jsonl) and prints a markdown
table. Usage: pose_probe.py [--out FILE] [--width W --height H] [--trace-frames N]."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, os.path.join(ROOT, "foveated-rendering-using-ray-tracing_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch  # noqa: E402  before libfovrt: one HIP runtime in the process (arm E's arrays live in tensors)
import fovrt  # noqa: E402
import pose_np as pn  # noqa: E402

ASSET_FILES = ("CedarCity.hdr", "grid.ppm", "bunny/bunny.PPM", "vokselia_spawn/vokselia_spawn.png")
WARMUP, TIMED, ROUNDS, CYCLE = 30, 60, 6, 8


def make(W, H, mode, have):
    t = fovrt.PathTracer(fovrt.Config(width=W, height=H, scene=fovrt.SCENE_BUNNY, mask_mode=fovrt.MASK_LOGPOLAR_SIGNED,
                                      spp=4, diffuse_max_depth=3, texture_mode=0 if have else 1))
    t.initialize()
    t.update_optix_variables(fovrt.Camera.preset(fovrt.SCENE_BUNNY, W, H))
    if mode == "latency":
        t.set_pipeline_mode(fovrt.PIPELINE_LATENCY)
    return t


def poses(models, pos):
    """CYCLE poses: the bunny turned about the vertical axis through its middle, the box slid along x."""
    out = []
    for i in range(CYCLE):
        m = pn.identities(len(models))
        for k, (name, first, n) in enumerate(models):
            p = pos[first:first + n].reshape(-1, 3).astype(np.float64)
            if name == "bunny":
                m[k] = pn.about(pn.rotation(1, 360.0 * i / CYCLE + 5.0), 0.5 * (p.min(0) + p.max(0)))
            elif name == "box":
                m[k] = pn.about(np.eye(3), (0, 0, 0), (0.05 * (i + 1), 0.0, 0.0))
        out.append(m)
    return out


def run(t, arm, ms, dev, n, frames, stream):
    for i in range(frames):
        k = i % CYCLE
        if arm == "P":
            t.set_model_transforms(ms[k], enqueue=True)
        elif arm == "E":
            t.update_geometry_enqueue(dev[k][0], ntris=n, normals=dev[k][1])
        t.frame(timing=False)
        if arm == "E":
            t.geometry_consumed(stream)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pose_probe.jsonl"))
    ap.add_argument("--width", type=int, default=3840)
    ap.add_argument("--height", type=int, default=2160)
    ap.add_argument("--trace-frames", type=int, default=0)
    args = ap.parse_args()
    W, H = args.width, args.height
    have = all(os.path.exists(os.path.join(fovrt.DEFAULT_ASSET_DIR, p)) for p in ASSET_FILES)
    if args.trace_frames:
        t = make(W, H, "throughput", have)
        t.enable_model_pose()
        models = t.models()
        ms = poses(models, t.scene_arrays()["pos"].reshape(-1, 3, 3))
        run(t, "P", ms, None, 0, args.trace_frames, None)
        t.synchronize()
        assert t.geometry_update_status() == (args.trace_frames, 0)
        t.destroy()
        return
    rows = []
    for mode in ("throughput", "latency"):
        ctx = {arm: make(W, H, mode, have) for arm in ("P", "E", "0")}
        ctx["P"].enable_model_pose()
        models = ctx["P"].models()
        a0 = ctx["P"].scene_arrays()
        pos, nrm = a0["pos"].reshape(-1, 3, 3), a0["nrm"].reshape(-1, 3, 3)
        n = pos.shape[0]
        ms = poses(models, pos)
        dev = []
        for m in ms:
            X, N = pn.pose_np(pos, nrm, models, m, a0["flags"])
            dev.append((torch.from_numpy(X.reshape(-1, 9)).to("cuda:0"), torch.from_numpy(N.reshape(-1, 9)).to("cuda:0")))
        torch.cuda.synchronize()
        stream = torch.cuda.current_stream()
        # the two arms render the same scene: one pose each way, compared in bytes
        ctx["P"].set_model_transforms(ms[1], enqueue=True)
        ctx["E"].update_geometry_enqueue(dev[1][0], ntris=n, normals=dev[1][1])
        p, e = ctx["P"].scene_arrays(), ctx["E"].scene_arrays()
        assert p["pos"].tobytes() == e["pos"].tobytes() and p["nrm"].tobytes() == e["nrm"].tobytes()
        for r in range(ROUNDS):
            order = ("P", "E", "0") if r < ROUNDS // 2 else ("0", "E", "P")
            for arm in order:
                t = ctx[arm]
                run(t, arm, ms, dev, n, WARMUP, stream)
                t.synchronize()
                t0 = time.perf_counter()
                run(t, arm, ms, dev, n, TIMED, stream)
                t.synchronize()
                dt = time.perf_counter() - t0
                row = dict(mode=mode, arm=arm, round=r, width=W, height=H, tris=n, models=len(models), frames=TIMED,
                           fps=TIMED / dt, ms_per_frame=1e3 * dt / TIMED)
                print(json.dumps(row), flush=True)
                rows.append(row)
        for arm in ("P", "E"):
            applied, rejected = ctx[arm].geometry_update_status()
            assert (applied, rejected) == (1 + ROUNDS * (WARMUP + TIMED), 0), (arm, applied, rejected)
        torch.cuda.synchronize()
        for t in ctx.values():
            t.destroy()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        for row in rows:
            f.write(json.dumps(row) + "\n")
    print("\n| mode | arm | fps per round | median | min | max | spread (max - min) |")
    print("|---|---|---|---|---|---|---|")
    for mode in ("throughput", "latency"):
        for arm in ("P", "E", "0"):
            v = [row["fps"] for row in rows if row["mode"] == mode and row["arm"] == arm]
            print(f"| {mode} | {arm} | {' '.join(f'{x:.1f}' for x in v)} | {float(np.median(v)):.1f} | {min(v):.1f} | "
                  f"{max(v):.1f} | {max(v) - min(v):.1f} |")


if __name__ == "__main__":
    main()
