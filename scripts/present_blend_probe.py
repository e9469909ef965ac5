#!/usr/bin/env python3
"""Blended present on the 4K bunny (MEASUREMENTS.md "Blended present"): what the gaze-contingent blend of SIBSON and
ATROUS costs beside the plain present, and that the loops which existed before it keep their rate.

  present_blend_probe.py fps [--rounds R] [--steps K] [--warmup W] [--windows N] [--parent LIB]
      frames per second of the pipelined loop (throughput mode, the bench workload, scripts/present_probe.py's
      protocol) in these forms, three slots in use, ticket k - 2 taken after ticket k:
        plain       fr_frame(NULL) alone
        present     + fr_present_enqueue(ATROUS) every frame
        identity    + fr_present_enqueue_warped(ATROUS), h = identity, 3840 x 2160
        blend       + fr_present_enqueue_blended, the default blend (fr_present_blend_default)
        blend_half  + the same around the same gaze with radii that put half the screen's texels in the ramp
        blend_turn2 + the default blend through the late reprojection of a 2 degree turn about the vertical axis
      With --parent the first three also run on that build of the library (FOVRT_LIB, FOVRT_LIB_OLDER=1) and, in a
      child of the same shape ("base": those three forms and no other), on this build; one child process per sample,
      the builds alternating. Each child reports the kernel's and the host copy's time of
      every present form from the slots' events (fr_present_times), medians over a window's frames.
  present_blend_probe.py one parent|base|all   (a child of the above; one JSON line)
"""
import argparse
import json
import os
import subprocess
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from present_probe import CHILD_TIMEOUT_S, H, W, tracer  # noqa: E402


def half_ramp_radii(np, gaze, r_in):
    """The outer radius (bisection, whole pixels) that puts half of the screen's texels strictly between the radii."""
    dx = (np.arange(W, dtype=np.float32) - np.float32(gaze[0]))[None, :]
    dy = (np.arange(H, dtype=np.float32) - np.float32(gaze[1]))[:, None]
    d2 = dx * dx + dy * dy
    inside = int((d2 <= np.float32(r_in) ** 2).sum())
    lo, hi = int(r_in), 2 * (W + H)
    while hi - lo > 1:
        mid = (lo + hi) // 2
        ramp = int((d2 < np.float32(mid) ** 2).sum()) - inside
        lo, hi = (mid, hi) if ramp < W * H // 2 else (lo, mid)
    return float(hi), (int((d2 < np.float32(hi) ** 2).sum()) - inside) / (W * H)


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

    def loop(enqueue):
        def run(n):
            tickets = []
            for _ in range(n):
                t.frame(timing=False)
                tickets.append(enqueue())
                while len(tickets) > 2:
                    take(tickets.pop(0))
            for tk in tickets:
                take(tk)
        return run

    def plain(n):
        for _ in range(n):
            t.frame(timing=False)

    ident = fovrt.PresentWarp.identity()
    forms = {"plain": plain, "present": loop(lambda: t.present(TN.ATROUS)),
             "identity": loop(lambda: t.present_warped(TN.ATROUS, ident))}
    if which == "all":
        cam = fovrt.Camera.preset(fovrt.SCENE_BUNNY, W, H)
        half = np.deg2rad(2.0) / 2
        disp = fovrt.Camera()
        disp.fovy, disp.znear, disp.zfar, disp.aspect = cam.fovy, cam.znear, cam.zfar, cam.aspect
        qw, qx, qy, qz = [float(v) for v in cam.rot]
        c, s = float(np.cos(half)), float(np.sin(half))  # cam.rot * (c, 0, s, 0): a turn about the camera's own y
        disp.setRotation((qw * c - qy * s, qx * c - qz * s, qy * c + qw * s, qz * c + qx * s))
        disp.setPosition(cam.pos)
        turn2 = fovrt.PresentWarp.from_poses(cam, disp, W, H)
        dflt = t.present_blend_default()
        r_out, frac = half_ramp_radii(np, dflt.gaze, dflt.inner_radius_px)
        wide = fovrt.PresentBlend(dflt.gaze, dflt.inner_radius_px, r_out)
        out["blend"] = {"gaze": [float(v) for v in dflt.gaze], "inner_radius_px": float(dflt.inner_radius_px),
                        "outer_radius_px": float(dflt.outer_radius_px), "half_outer_radius_px": r_out,
                        "half_ramp_fraction": round(frac, 4)}
        forms["blend"] = loop(lambda: t.present_blended(dflt))
        forms["blend_half"] = loop(lambda: t.present_blended(wide))
        forms["blend_turn2"] = loop(lambda: t.present_blended(dflt, turn2))
    t.present_enable(3, fovrt.FR_PRESENT_BGRA8)
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
                out.setdefault("pack_ms", {}).setdefault(name, []).append(round(float(np.median(a[:, 0])), 4))
                out.setdefault("copy_ms", {}).setdefault(name, []).append(round(float(np.median(a[:, 1])), 4))
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
    ap.add_argument("which", nargs="?", default="all", choices=["parent", "base", "all"])
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=30)
    ap.add_argument("--windows", type=int, default=3)
    ap.add_argument("--parent", default=None, help="the parent commit's build of the library, for the first three forms")
    args = ap.parse_args()
    if args.cmd == "one":
        return one(args.which, args.steps, args.warmup, args.windows)
    for _ in range(args.rounds):
        if args.parent:
            child("parent", args, args.parent)
            child("base", args)
        child("all", args)


if __name__ == "__main__":
    main()
