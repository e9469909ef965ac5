#!/usr/bin/env python3
"""Present on the 4K bunny (MEASUREMENTS.md "Present"): what delivering every frame to the host costs.

  present_probe.py fps [--rounds R] [--steps K] [--warmup W] [--windows N] [--parent LIB]
      frames per second of the pipelined loop (throughput mode, the bench workload) in four forms:
        plain    fr_frame(NULL) alone, nothing delivered (with --parent also on that build of the library:
                 FOVRT_LIB, FOVRT_LIB_OLDER=1, one child process per sample, alternating with this build's)
        present  fr_frame(NULL) + fr_present_enqueue(ATROUS) every frame, three slots; the consumer acquires and
                 releases ticket k - 2 after enqueueing ticket k, so every frame reaches the host
        read     fr_frame(NULL) + fr_read_buffer(ATROUS) every frame: the loop a caller had to write before
      A child of this build times the three forms in turn, --windows times over, each window --steps frames
      between two synchronisations after --warmup frames of that form; it also reports the pack kernel's and the
      host copy's time from the slots' events (fr_present_times), over every frame of the present windows.
  present_probe.py one plain|all   (a child of the above; one JSON line)
"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "foveated-rendering-using-ray-tracing_amd"))
W, H = 3840, 2160
CHILD_TIMEOUT_S = 240


def tracer(fovrt):
    assets = all(os.path.exists(os.path.join(fovrt.DEFAULT_ASSET_DIR, p))
                 for p in ("CedarCity.hdr", "grid.ppm", "bunny/bunny.PPM", "vokselia_spawn/vokselia_spawn.png"))
    t = fovrt.PathTracer(fovrt.Config(width=W, height=H, scene=fovrt.SCENE_BUNNY, mask_mode=fovrt.MASK_LOGPOLAR_SIGNED,
                                      spp=4, diffuse_max_depth=3, texture_mode=0 if assets else 1))
    t.initialize()
    t.update_optix_variables(fovrt.Camera.preset(fovrt.SCENE_BUNNY, W, H))
    return t


def one(which, steps, warmup, windows):
    import numpy as np
    import torch  # noqa: F401  (the process's HIP runtime is torch's, as in the suite and the bench)
    import fovrt
    t = tracer(fovrt)
    TN = fovrt.TextureName
    lib = fovrt.load_library()
    out = {"which": which, "lib": os.environ.get("FOVRT_LIB", "this build"), "steps": steps, "warmup": warmup}
    host = np.empty((H, W, 4), np.float32)
    pack_ms, copy_ms = [], []

    def plain(n):
        for _ in range(n):
            t.frame(timing=False)

    def present(n):
        tickets = []
        for _ in range(n):
            t.frame(timing=False)
            tickets.append(t.present(TN.ATROUS))
            if len(tickets) > 2:
                take(tickets.pop(0))
        for tk in tickets:
            take(tk)

    def take(tk):
        img = t.present_acquire(tk)
        assert img[0, 0, 3] == 255
        tm = t.present_times(tk)
        pack_ms.append(tm["pack_ms"]); copy_ms.append(tm["copy_ms"])
        t.present_release(tk)

    def read(n):
        for _ in range(n):
            t.frame(timing=False)
            rc = lib.fr_read_buffer(t._ctx, int(TN.ATROUS), C.c_void_p(host.ctypes.data), host.nbytes)
            assert rc == 0

    forms = {"plain": plain} if which == "plain" else {"plain": plain, "present": present, "read": read}
    if "present" in forms:
        t.present_enable(3, fovrt.FR_PRESENT_BGRA8)
    fps = {k: [] for k in forms}
    for _ in range(windows):
        for name, fn in forms.items():
            fn(warmup)
            t.synchronize()
            del pack_ms[:], copy_ms[:]
            t0 = time.perf_counter()
            fn(steps)
            t.synchronize()
            fps[name].append(round(steps / (time.perf_counter() - t0), 2))
            if name == "present":
                out.setdefault("pack_ms", []).append(round(float(np.median(pack_ms)), 4))
                out.setdefault("copy_ms", []).append(round(float(np.median(copy_ms)), 4))
                out.setdefault("copy_ms_max", []).append(round(float(np.max(copy_ms)), 4))
    out["fps"] = fps
    out["bytes_per_frame"] = {"present": W * H * 4, "read": W * H * 16}
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
    return json.loads(line)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("cmd", choices=["fps", "one"])
    ap.add_argument("which", nargs="?", default="all", choices=["plain", "all"])
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=30)
    ap.add_argument("--windows", type=int, default=3)
    ap.add_argument("--parent", default=None, help="another build of the library, for the plain loop beside this one's")
    args = ap.parse_args()
    if args.cmd == "one":
        return one(args.which, args.steps, args.warmup, args.windows)
    for _ in range(args.rounds):
        if args.parent:
            child("plain", args, args.parent)
        child("all", args)


if __name__ == "__main__":
    main()
