#!/usr/bin/env python3
"""Reprojected present on the 4K bunny (MEASUREMENTS.md "Reprojected present"): what the depth-aware splat costs beside
the plain and the warped present.

  present_reproject_probe.py fps [--rounds R] [--steps K] [--warmup W] [--windows N] [--parent LIB]
      frames per second of the pipelined loop (throughput mode, the bench workload, scripts/present_probe.py's
      protocol) in these forms, every present on ATROUS with three slots, ticket k - 2 taken after ticket k:
        plain      fr_frame(NULL) alone
        present    + fr_present_enqueue every frame
        turn2      + fr_present_enqueue_warped, the late reprojection of a 2 degree turn about the vertical axis
        reproject  + fr_present_enqueue_reprojected to the rendered pose itself (every hit lands on or next to its place)
        moved      + fr_present_enqueue_reprojected to a pose turned by 2 degrees and moved 0.05 units sideways and
                   0.05 units forward
        idle       fr_frame(NULL) alone on a context that presents but has not enabled the reprojection (this build
                   only, timed before the enable; `plain` is the same loop after it, and on the parent build the loop of
                   a context that presents)
      With --parent the first three also run on that build of the library (FOVRT_LIB, FOVRT_LIB_OLDER=1), one child
      process per sample, alternating with this build's. Each child reports the kernels' time (clear, splat and resolve
      together for the reprojected forms) and the host copy's time of every present form from the slots' events
      (fr_present_times), medians over a window's frames.
  present_reproject_probe.py kernels [--steps K]
      one process, `moved` and `turn2` and `present` in turn, K frames each: run it under a kernel trace to split the
      reprojected present's time between k_present_splat and k_present_resolve.
  present_reproject_probe.py one parent|all   (a child of the above; one JSON line)
"""
import argparse
import json
import os
import subprocess
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from present_probe import CHILD_TIMEOUT_S, H, W, tracer  # noqa: E402


def display(fovrt, cam, deg, move):
    """A copy of the camera turned by `deg` about its own y and moved by `move` (right, up, forward)."""
    import numpy as np
    half = np.deg2rad(deg) / 2
    disp = fovrt.Camera()
    disp.fovy, disp.znear, disp.zfar, disp.aspect = cam.fovy, cam.znear, cam.zfar, cam.aspect
    qw, qx, qy, qz = [float(v) for v in cam.rot]
    c, s = float(np.cos(half)), float(np.sin(half))  # cam.rot * (c, 0, s, 0)
    disp.setRotation((qw * c - qy * s, qx * c - qz * s, qy * c + qw * s, qz * c + qx * s))
    V = cam.getVMat().astype(np.float64)
    disp.setPosition(cam.pos + (move[0] * V[0, :3] + move[1] * V[1, :3] - move[2] * V[2, :3]).astype(np.float32))
    return disp


def forms_of(fovrt, t, which, times):
    TN = fovrt.TextureName

    def take(tk):
        img = t.present_acquire(tk)
        assert img[0, 0, 3] == 255
        tm = t.present_times(tk)
        times.append((tm["pack_ms"], tm["copy_ms"]))
        t.present_release(tk)

    def loop(enqueue, depth):
        def run(n):
            tickets = []
            for _ in range(n):
                t.frame(timing=False)
                tickets += enqueue()
                while len(tickets) > depth:
                    take(tickets.pop(0))
            for tk in tickets:
                take(tk)
        return run

    cam = fovrt.Camera.preset(fovrt.SCENE_BUNNY, W, H)
    turn2 = fovrt.PresentWarp.from_poses(cam, display(fovrt, cam, 2.0, (0, 0, 0)), W, H)
    forms = {"plain": loop(lambda: [], 0), "present": loop(lambda: [t.present(TN.ATROUS)], 2),
             "turn2": loop(lambda: [t.present_warped(TN.ATROUS, turn2)], 2)}
    if which == "all":
        same = fovrt.PresentReproject.from_poses(cam, cam, W, H)
        moved = fovrt.PresentReproject.from_poses(cam, display(fovrt, cam, 2.0, (0.05, 0.0, 0.05)), W, H)
        forms["reproject"] = loop(lambda: [t.present_reprojected(TN.ATROUS, same)], 2)
        forms["moved"] = loop(lambda: [t.present_reprojected(TN.ATROUS, moved)], 2)
    return forms


def one(which, steps, warmup, windows):
    import numpy as np
    import torch  # noqa: F401  (the process's HIP runtime is torch's, as in the suite and the bench)
    import fovrt
    t = tracer(fovrt)
    out = {"which": which, "lib": os.environ.get("FOVRT_LIB", "this build"), "steps": steps, "warmup": warmup}
    times = []
    forms = forms_of(fovrt, t, which, times)
    fps = {k: [] for k in forms}
    if which == "all":  # before the reprojection is enabled: a context that presents and has no key image
        t.present_enable(3, fovrt.FR_PRESENT_BGRA8)
        fps["idle"] = []
        for _ in range(windows):
            forms["plain"](warmup)
            t.synchronize()
            t0 = time.perf_counter()
            forms["plain"](steps)
            t.synchronize()
            fps["idle"].append(round(steps / (time.perf_counter() - t0), 2))
        t.present_reproject_enable()
    else:
        t.present_enable(3, fovrt.FR_PRESENT_BGRA8)
    for _ in range(windows):
        for name, fn in forms.items():
            fn(warmup)
            t.synchronize()
            del times[:]
            t0 = time.perf_counter()
            fn(steps)
            t.synchronize()
            fps[name].append(round(steps / (time.perf_counter() - t0), 2))
            if times:
                a = np.array(times)
                out.setdefault("pack_ms", {}).setdefault(name, []).append(round(float(np.median(a[:, 0])), 4))
                out.setdefault("copy_ms", {}).setdefault(name, []).append(round(float(np.median(a[:, 1])), 4))
    out["fps"] = fps
    t.destroy()
    print(json.dumps(out), flush=True)


def kernels(steps):
    import torch  # noqa: F401
    import fovrt
    t = tracer(fovrt)
    times = []
    forms = forms_of(fovrt, t, "all", times)
    t.present_enable(3, fovrt.FR_PRESENT_BGRA8)
    t.present_reproject_enable()
    for name in ("present", "turn2", "moved"):
        forms[name](steps)
        t.synchronize()
    t.destroy()
    print(json.dumps({"kernels": "done", "steps": steps}), flush=True)


def child(which, args, lib=None):
    env = dict(os.environ)
    if lib:
        env["FOVRT_LIB"], env["FOVRT_LIB_OLDER"] = lib, "1"
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "one", which, "--steps", str(args.steps), "--warmup",
                        str(args.warmup), "--windows", str(args.windows)], env=env, capture_output=True, text=True,
                       timeout=CHILD_TIMEOUT_S)
    if r.returncode != 0:
        sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
        raise SystemExit(f"child '{which}' ended with {r.returncode}: stopping")
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1]
    print(line, flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("cmd", choices=["fps", "one", "kernels"])
    ap.add_argument("which", nargs="?", default="all", choices=["parent", "all"])
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=30)
    ap.add_argument("--windows", type=int, default=3)
    ap.add_argument("--parent", default=None, help="the parent commit's build of the library, for the first three forms")
    args = ap.parse_args()
    if args.cmd == "one":
        return one(args.which, args.steps, args.warmup, args.windows)
    if args.cmd == "kernels":
        return kernels(args.steps)
    for _ in range(args.rounds):
        if args.parent:
            child("parent", args, args.parent)
        child("all", args)


if __name__ == "__main__":
    main()
