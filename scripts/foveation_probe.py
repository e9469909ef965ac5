#!/usr/bin/env python3
"""Foveation control on the 4K bunny (MEASUREMENTS.md "Foveation control").

  foveation_probe.py fps [--rounds R] [--steps K] [--warmup W] [--parent LIB]
      pipelined frames per second, both pipeline modes, of: mode 5 without a budget; mode 5 with the budget set to the
      ray count the signed log-polar mode produces on that view; a fresh caller mask enqueued before every frame. Every
      sample is one child process; with --parent (another build of the library: FOVRT_LIB, FOVRT_LIB_OLDER=1) each is
      taken beside that build's signed log-polar line, the two alternating.
  foveation_probe.py one CONFIG   (a child of the above: logpolar | ecc | ecc_budget | caller; one JSON line)
  foveation_probe.py kernels
      launches every kernel of the feature and the log-polar pair a few times at 4K, for a kernel trace:
      rocprofv3 --kernel-trace --stats -f csv -d DIR -o run -- python scripts/foveation_probe.py kernels
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "foveated-rendering-using-ray-tracing_amd"))
W, H = 3840, 2160


def tracer(fovrt):
    assets = all(os.path.exists(os.path.join(fovrt.DEFAULT_ASSET_DIR, p))
                 for p in ("CedarCity.hdr", "grid.ppm", "bunny/bunny.PPM", "vokselia_spawn/vokselia_spawn.png"))
    t = fovrt.PathTracer(fovrt.Config(width=W, height=H, scene=fovrt.SCENE_BUNNY, mask_mode=fovrt.MASK_LOGPOLAR_SIGNED,
                                      spp=4, diffuse_max_depth=3, texture_mode=0 if assets else 1))
    t.initialize()
    t.update_optix_variables(fovrt.Camera.preset(fovrt.SCENE_BUNNY, W, H))
    return t


def one(config, steps, warmup):
    import numpy as np
    import torch
    import fovrt
    t = tracer(fovrt)
    out = {"config": config, "lib": os.environ.get("FOVRT_LIB", "this build")}
    masks = None
    if config != "logpolar":
        for _ in range(3):
            t.frame(timing=False)
        out["logpolar_count"] = t.ray_count()
    if config in ("ecc", "ecc_budget"):
        t.set_mask_mode(fovrt.MASK_ECCENTRIC)
        if config == "ecc_budget":
            t.set_foveation(ray_budget=out["logpolar_count"])
    elif config == "caller":
        rng = np.random.default_rng(1)
        masks = [torch.from_numpy((rng.random(W * H) < 0.1).astype(np.uint8)).to("cuda:0") for _ in range(4)]
        torch.cuda.synchronize()
        t.enable_sampling_mask()
        t.set_sampling_mask(masks[0])
        t.set_mask_mode(fovrt.MASK_CALLER)
    for name, mode in (("throughput", fovrt.PIPELINE_THROUGHPUT), ("latency", fovrt.PIPELINE_LATENCY)):
        t.set_pipeline_mode(mode)
        for k in range(warmup + steps):
            if k == warmup:
                t.synchronize()
                t0 = time.perf_counter()
            if masks:
                t.set_sampling_mask(masks[k % len(masks)], enqueue=True)
            t.frame(timing=False)
        t.synchronize()
        out[name + "_fps"] = round(steps / (time.perf_counter() - t0), 2)
    out["count"] = t.ray_count()
    if config == "ecc_budget":
        out["status"] = t.foveation_status()
    t.destroy()
    print(json.dumps(out), flush=True)


def kernels():
    import numpy as np
    import torch
    import fovrt
    t = tracer(fovrt)
    t.geometry_launch()
    m = torch.from_numpy((np.random.default_rng(1).random(W * H) < 0.1).astype(np.uint8)).to("cuda:0")
    torch.cuda.synchronize()
    t.enable_sampling_mask()
    for k in range(10):
        t.set_gaze(W / 2 + 8 * k, H / 2 / 1.25)  # another gaze: both cached masks are generated again
        t.set_mask_mode(fovrt.MASK_LOGPOLAR_SIGNED)
        t.sampling_launch(); t.optimize_launch()
        t.set_mask_mode(fovrt.MASK_ECCENTRIC)
        t.set_foveation(ray_budget=0)
        t.sampling_launch(); t.optimize_launch()
        t.set_foveation(ray_budget=800000)
        t.sampling_launch(); t.optimize_launch()
        t.sampling_launch()
        t.set_sampling_mask(m, enqueue=True)
        t.set_mask_mode(fovrt.MASK_CALLER)
        t.sampling_launch()
    t.synchronize()
    t.destroy()


def fps(rounds, steps, warmup, parent):
    def child(config, lib=None):
        env = dict(os.environ)
        if lib:
            env.update(FOVRT_LIB=lib, FOVRT_LIB_OLDER="1")
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "one", config, "--steps", str(steps), "--warmup",
                            str(warmup)], env=env, capture_output=True, text=True, timeout=240)
        if r.returncode:
            print(r.stdout[-2000:], r.stderr[-2000:], file=sys.stderr)
            sys.exit(r.returncode)  # nothing more is started on the device after a child that failed
        line = [l for l in r.stdout.splitlines() if l.startswith("{")][-1]
        print(line, flush=True)
        return json.loads(line)

    for config in ("ecc", "ecc_budget", "caller"):
        rows = {"new": [], "parent": []}
        for _ in range(rounds):
            rows["new"].append(child(config))
            rows["parent"].append(child("logpolar", parent) if parent else child("logpolar"))
        for mode in ("throughput", "latency"):
            a = sorted(r[mode + "_fps"] for r in rows["new"])
            b = sorted(r[mode + "_fps"] for r in rows["parent"])
            print(f"{config:10s} {mode:10s} fps {a}  count {rows['new'][-1]['count']}  |  "
                  f"{'parent' if parent else 'this build'} logpolar10 fps {b}  count {rows['parent'][-1]['count']}",
                  flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=["fps", "one", "kernels"])
    ap.add_argument("config", nargs="?", default="ecc")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=60)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--parent", default=None)
    a = ap.parse_args()
    if a.what == "one":
        one(a.config, a.steps, a.warmup)
    elif a.what == "kernels":
        kernels()
    else:
        fps(a.rounds, a.steps, a.warmup, a.parent)
