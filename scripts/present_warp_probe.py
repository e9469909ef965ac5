#!/usr/bin/env python3
"""Warped present on the 4K bunny (MEASUREMENTS.md "Warped present"): what the homography costs beside the plain present.

  present_warp_probe.py fps [--rounds R] [--steps K] [--warmup W] [--windows N] [--parent LIB]
      frames per second of the pipelined loop (throughput mode, the bench workload, scripts/present_probe.py's
      protocol) in these forms, every present on ATROUS with three slots, ticket k - 2 taken after ticket k:
        plain     fr_frame(NULL) alone
        present   + fr_present_enqueue every frame
        identity  + fr_present_enqueue_warped, h = identity, 3840 x 2160
        turn2     + fr_present_enqueue_warped, the late reprojection of a 2 degree turn about the vertical axis
        pair      + two warped presents a frame: the whole image at 1920 x 1080 and a 1024 x 1024 crop around the
                  screen's centre (six slots)
      With --parent the first two also run on that build of the library (FOVRT_LIB, FOVRT_LIB_OLDER=1), one child
      process per sample, alternating with this build's. Each child reports the kernel's and the host copy's time of
      every present form from the slots' events (fr_present_times), medians over a window's frames.
  present_warp_probe.py one parent|all   (a child of the above; one JSON line)
"""
import argparse
import json
import os
import subprocess
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from present_probe import CHILD_TIMEOUT_S, H, W, tracer  # noqa: E402


def one(which, steps, warmup, windows):
    import numpy as np
    import torch  # noqa: F401  (the process's HIP runtime is torch's, as in the suite and the bench)
    import fovrt
    t = tracer(fovrt)
    TN = fovrt.TextureName
    out = {"which": which, "lib": os.environ.get("FOVRT_LIB", "this build"), "steps": steps, "warmup": warmup}
    times = []

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

    forms = {"plain": loop(lambda: [], 0), "present": loop(lambda: [t.present(TN.ATROUS)], 2)}
    if which == "all":
        PWp = fovrt.PresentWarp
        cam = fovrt.Camera.preset(fovrt.SCENE_BUNNY, W, H)
        half = np.deg2rad(2.0) / 2
        disp = fovrt.Camera()
        disp.fovy, disp.znear, disp.zfar, disp.aspect = cam.fovy, cam.znear, cam.zfar, cam.aspect
        qw, qx, qy, qz = [float(v) for v in cam.rot]
        c, s = float(np.cos(half)), float(np.sin(half))  # cam.rot * (c, 0, s, 0): a turn about the camera's own y
        disp.setRotation((qw * c - qy * s, qx * c - qz * s, qy * c + qw * s, qz * c + qx * s))
        disp.setPosition(cam.pos)
        ident, turn2 = PWp.identity(), PWp.from_poses(cam, disp, W, H)
        small, fovea = PWp.scale(W, H, W // 2, H // 2), PWp.crop((W - 1024) // 2, (H - 1024) // 2, 1024, 1024)
        out["turn2_h"] = [float(v) for v in turn2.h]
        forms["identity"] = loop(lambda: [t.present_warped(TN.ATROUS, ident)], 2)
        forms["turn2"] = loop(lambda: [t.present_warped(TN.ATROUS, turn2)], 2)
        forms["pair"] = loop(lambda: [t.present_warped(TN.ATROUS, small), t.present_warped(TN.ATROUS, fovea)], 4)
    t.present_enable(6, fovrt.FR_PRESENT_BGRA8)
    fps = {k: [] for k in forms}
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
                k = 2 if name == "pair" else 1  # pair: the half-size image and the crop alternate
                for j in range(k):
                    key = name if k == 1 else name + ("_half", "_crop")[j]
                    out.setdefault("pack_ms", {}).setdefault(key, []).append(round(float(np.median(a[j::k, 0])), 4))
                    out.setdefault("copy_ms", {}).setdefault(key, []).append(round(float(np.median(a[j::k, 1])), 4))
    out["fps"] = fps
    t.destroy()
    print(json.dumps(out), flush=True)


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
    ap.add_argument("cmd", choices=["fps", "one"])
    ap.add_argument("which", nargs="?", default="all", choices=["parent", "all"])
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=30)
    ap.add_argument("--windows", type=int, default=3)
    ap.add_argument("--parent", default=None, help="the parent commit's build of the library, for the first two forms")
    args = ap.parse_args()
    if args.cmd == "one":
        return one(args.which, args.steps, args.warmup, args.windows)
    for _ in range(args.rounds):
        if args.parent:
            child("parent", args, args.parent)
        child("all", args)


if __name__ == "__main__":
    main()
