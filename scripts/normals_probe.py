"""What shading normals that follow the geometry add to a position update, per scene (bunny, vokselia) at the
default detail: six calls in a row, in one process, of

  fr_recompute_normals                                    (its own *ms; the context's first call on its own row)
  fr_update_geometry(device, FR_BVH_REFIT, FR_NORMALS_RECOMPUTE)   (wall)
  fr_update_positions(device, FR_BVH_REFIT)                        (wall)
  fr_update_positions(device, FR_BVH_REBUILD)                      (wall, on a second context with the LBVH)

The refit's value is that it costs less than the rebuild, so the update with recompute is to be read against the
last two as measured here, in the same run.

Writes one JSON line per measurement to --out (default profiles/normals_probe.jsonl) and prints a markdown table.
Usage: normals_probe.py [--out FILE] [scene ...] (default 1 2)."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, os.path.join(ROOT, "foveated-rendering-using-ray-tracing_amd"))
import torch  # noqa: E402  before libfovrt: one HIP runtime in the process (the positions live in a tensor)
import fovrt  # noqa: E402

W, H = 1024, 1024
ASSET_FILES = ("CedarCity.hdr", "grid.ppm", "bunny/bunny.PPM", "vokselia_spawn/vokselia_spawn.png")


def make(scene, builder):
    have = all(os.path.exists(os.path.join(fovrt.DEFAULT_ASSET_DIR, p)) for p in ASSET_FILES)
    t = fovrt.PathTracer(fovrt.Config(width=W, height=H, scene=scene, mask_mode=fovrt.MASK_LOGPOLAR_SIGNED, spp=4,
                                      diffuse_max_depth=3, bvh_builder=builder, texture_mode=0 if have else 1))
    t.initialize()
    t.update_optix_variables(fovrt.Camera.preset(scene, W, H))
    return t


def deform(base, amp, bbox):
    """refit_probe.py's deformation: two sine periods across the box; amp in scene units."""
    lo, ext = bbox[:3], np.maximum(bbox[3:] - bbox[:3], np.float32(1e-6))
    pos = base.copy()
    k = np.float32(4.0 * np.pi)
    pos[..., 1] += np.float32(amp) * np.sin(k * (base[..., 0] - lo[0]) / ext[0]).astype(np.float32)
    pos[..., 0] += np.float32(amp) * np.sin(k * (base[..., 2] - lo[2]) / ext[2]).astype(np.float32)
    return pos


def timed(fn):
    out = []
    for _ in range(6):
        t0 = time.perf_counter()
        fn()
        out.append((time.perf_counter() - t0) * 1e3)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "normals_probe.jsonl"))
    ap.add_argument("scenes", nargs="*", type=int, default=[1, 2])
    args = ap.parse_args()
    rows = []

    def emit(**kw):
        rows.append(kw)
        print(json.dumps(kw), flush=True)

    for scene in args.scenes:
        a, b = make(scene, 0), make(scene, 1)  # a: host SAH tree, refitted; b: LBVH, rebuilt
        arrays = a.scene_arrays()
        base = arrays["pos"].reshape(-1, 3, 3).copy()
        bbox = np.asarray(arrays["bbox"], np.float32)
        n = base.shape[0]
        cv, nv = a.normal_groups()
        valence = np.bincount(cv[cv >= 0], minlength=nv)
        common = dict(scene=scene, tris=n, vertices=nv, max_valence=int(valence.max()))
        pos = deform(base, 0.02 * float(np.linalg.norm(bbox[3:] - bbox[:3])), bbox)
        dev = torch.from_numpy(pos.reshape(-1, 9)).to("cuda:0")
        torch.cuda.synchronize()
        a.set_positions_device(dev.data_ptr(), n, update="refit")  # the refit's first call is not the subject
        t0 = time.perf_counter()
        first_ms = a.recompute_normals()  # the context's first launch of the rule's kernels
        emit(call="fr_recompute_normals, first call of the context (its ms, wall)",
             ms=[first_ms, (time.perf_counter() - t0) * 1e3], **common)
        emit(call="fr_recompute_normals (its ms)", ms=[a.recompute_normals() for _ in range(6)], **common)
        emit(call="fr_update_geometry device refit recompute",
             ms=timed(lambda: a.set_positions_device(dev.data_ptr(), n, update="refit", normals="recompute")), **common)
        emit(call="fr_update_positions device refit",
             ms=timed(lambda: a.set_positions_device(dev.data_ptr(), n, update="refit")), **common)
        emit(call="fr_update_positions device rebuild",
             ms=timed(lambda: b.set_positions_device(dev.data_ptr(), n, update="rebuild")), **common)
        a.destroy(); b.destroy()

    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        for r in rows:
            f.write(json.dumps(r) + "\n")

    print("\n| scene | triangles | vertices | call | calls, ms | median |")
    print("|---|---|---|---|---|---|")
    for r in rows:
        print(f"| {r['scene']} | {r['tris']} | {r['vertices']} | {r['call']} | {' '.join(f'{m:.3f}' for m in r['ms'])} | "
              f"{statistics.median(r['ms']):.3f} |")


if __name__ == "__main__":
    main()
