"""What the motion form of the G-buffer and of the sampling stage costs (fr_set_motion_reprojection): the bench
workload's frame (bunny 4K, 4 spp, GI 3, signed log-polar mask), a refit from device memory before every frame,
and each stage timed alone by its own launch call (fr_geometry_launch / fr_sampling_launch, HIP events around the
stage, as DESIGN.md §4 times stages). The two arms alternate inside one process and one context, in swapped order
every iteration: the same positions, the same tree, the feature on (the motion kernels) or off (the plain ones).
Three warm-up iterations, then the median of ten.

Writes one JSON line per (arm, stage) to --out (default profiles/motion_probe.jsonl) and prints a markdown table.
Usage: motion_probe.py [--out FILE] [--width W --height H]."""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, os.path.join(ROOT, "foveated-rendering-using-ray-tracing_amd"))
import torch  # noqa: E402  before libfovrt: one HIP runtime in the process (the positions live in a tensor)
import fovrt  # noqa: E402

ASSET_FILES = ("CedarCity.hdr", "grid.ppm", "bunny/bunny.PPM", "vokselia_spawn/vokselia_spawn.png")
WARMUP, TIMED = 3, 10


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "motion_probe.jsonl"))
    ap.add_argument("--width", type=int, default=3840)
    ap.add_argument("--height", type=int, default=2160)
    args = ap.parse_args()
    W, H = args.width, args.height
    have = all(os.path.exists(os.path.join(fovrt.DEFAULT_ASSET_DIR, p)) for p in ASSET_FILES)
    t = fovrt.PathTracer(fovrt.Config(width=W, height=H, scene=fovrt.SCENE_BUNNY, mask_mode=fovrt.MASK_LOGPOLAR_SIGNED,
                                      spp=4, diffuse_max_depth=3, texture_mode=0 if have else 1))
    t.initialize()
    t.update_optix_variables(fovrt.Camera.preset(fovrt.SCENE_BUNNY, W, H))
    base = t.scene_arrays()["pos"].reshape(-1, 3, 3).copy()
    n = base.shape[0]
    dev = []
    for phase in (0.0, 1.0):  # two poses of one wave: every update moves every vertex
        pos = base.copy()
        pos[..., 1] += np.float32(0.05) * np.sin(np.float32(3.0) * base[..., 0] + np.float32(phase)).astype(np.float32)
        dev.append(torch.from_numpy(pos.reshape(-1, 9)).to("cuda:0"))
    torch.cuda.synchronize()
    ms = {(arm, stage): [] for arm in ("plain", "motion") for stage in ("geometry", "sampling")}
    for i in range(WARMUP + TIMED):
        arms = ("motion", "plain") if i & 1 else ("plain", "motion")
        for arm in arms:
            t.set_motion_reprojection(arm == "motion")
            t.set_positions_device(dev[i & 1].data_ptr(), n, update="refit")
            g = t.geometry_launch()
            s = t.sampling_launch()
            t.optimize_launch()
            t.shading_launch()  # the rest of the frame: the depth pair rotates as in a frame loop
            if i >= WARMUP:
                ms[(arm, "geometry")].append(g)
                ms[(arm, "sampling")].append(s)
    t.destroy()
    rows = [dict(width=W, height=H, tris=n, arm=arm, stage=stage, ms=v, median=statistics.median(v))
            for (arm, stage), v in ms.items()]
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        for r in rows:
            print(json.dumps(r), flush=True)
            f.write(json.dumps(r) + "\n")
    print("\n| stage | arm | calls, ms | median | min |")
    print("|---|---|---|---|---|")
    for r in rows:
        print(f"| {r['stage']} | {r['arm']} | {' '.join(f'{m:.3f}' for m in r['ms'])} | {r['median']:.3f} | "
              f"{min(r['ms']):.3f} |")


if __name__ == "__main__":
    main()
