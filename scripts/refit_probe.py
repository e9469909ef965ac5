"""Refit against rebuild for moving geometry, at 4K, per scene (bunny, vokselia):

 (a) wall time of six fr_refit_bvh and six fr_rebuild_bvh calls in a row, and of whole position updates
     (fr_update_positions: host / device memory x rebuild / refit, six each);
 (b) tree quality: fr_bvh_sah_cost and the live megakernel time (fr_kernel_timing's shade_paths_ms over 20
     pipelined frames) of the untouched host SAH tree, of that tree refitted under a smooth sine deformation at
     amplitudes 0, 0.5 %, 2 % and 10 % of the scene-box diagonal, and of an LBVH rebuild over the same positions
     (a second context fed the same arrays, so both render the same frames).

Writes one JSON line per measurement to --out (default profiles/refit_probe.jsonl) and prints a markdown table.
Usage: refit_probe.py [--out FILE] [scene ...] (default 1 2)."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, os.path.join(ROOT, "foveated-rendering-using-ray-tracing_amd"))
try:
    import torch  # before libfovrt: one HIP runtime in the process (device-memory updates use a tensor)
except ImportError:
    torch = None
import fovrt  # noqa: E402

W, H, FRAMES, WARM = 3840, 2160, 20, 5
AMPLITUDES = (0.0, 0.005, 0.02, 0.10)
ASSET_FILES = ("CedarCity.hdr", "grid.ppm", "bunny/bunny.PPM", "vokselia_spawn/vokselia_spawn.png")


def make(scene, builder):
    have = all(os.path.exists(os.path.join(fovrt.DEFAULT_ASSET_DIR, p)) for p in ASSET_FILES)
    t = fovrt.PathTracer(fovrt.Config(width=W, height=H, scene=scene, mask_mode=fovrt.MASK_LOGPOLAR_SIGNED, spp=4,
                                      diffuse_max_depth=3, bvh_builder=builder, texture_mode=0 if have else 1))
    t.initialize()
    t.update_optix_variables(fovrt.Camera.preset(scene, W, H))
    return t


def deform(base, amp, bbox):
    """Two sine periods across the box: y moves with x, x moves with z; amp in scene units."""
    lo, ext = bbox[:3], np.maximum(bbox[3:] - bbox[:3], np.float32(1e-6))
    pos = base.copy()
    k = np.float32(4.0 * np.pi)
    pos[..., 1] += np.float32(amp) * np.sin(k * (base[..., 0] - lo[0]) / ext[0]).astype(np.float32)
    pos[..., 0] += np.float32(amp) * np.sin(k * (base[..., 2] - lo[2]) / ext[2]).astype(np.float32)
    return pos


def trace_ms(t):
    """Mean shade_paths_ms of FRAMES pipelined frames after WARM frames over the current geometry."""
    for _ in range(WARM):
        t.frame(False)
    t.synchronize()
    t.kernel_timing(True)
    for _ in range(FRAMES):
        t.frame(False)
    t.synchronize()
    k = t.kernel_times()
    t.kernel_timing(False)
    return k["shade_paths_ms"] / max(k["frames"], 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "refit_probe.jsonl"))
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
        diag = float(np.linalg.norm(bbox[3:] - bbox[:3]))
        n = base.shape[0]
        common = dict(scene=scene, tris=n, nodes_sah=arrays["bvh_nodes"], nodes_lbvh=b.scene_arrays()["bvh_nodes"])
        # (b) quality
        emit(kind="quality", tree="host SAH, untouched", amplitude=None, cost=a.bvh_sah_cost(),
             shade_paths_ms=trace_ms(a), **common)
        for amp in AMPLITUDES:
            pos = deform(base, amp * diag, bbox)
            a.set_positions(pos, update="refit")
            b.set_positions(pos)
            emit(kind="quality", tree="host SAH, refitted", amplitude=amp, cost=a.bvh_sah_cost(),
                 shade_paths_ms=trace_ms(a), **common)
            emit(kind="quality", tree="LBVH rebuild", amplitude=amp, cost=b.bvh_sah_cost(), shade_paths_ms=trace_ms(b),
                 **common)
        # (a) wall times: the tree calls alone, then whole updates (a keeps the SAH topology until its rebuilds)
        pos = deform(base, 0.02 * diag, bbox)
        emit(kind="wall", call="fr_refit_bvh", ms=[a.refit_bvh() for _ in range(6)], **common)

        def timed(fn):
            out = []
            for _ in range(6):
                t0 = time.perf_counter()
                fn()
                out.append((time.perf_counter() - t0) * 1e3)
            return out

        emit(kind="wall", call="fr_update_positions host refit", ms=timed(lambda: a.set_positions(pos, update="refit")),
             **common)
        if torch is not None:
            dev = torch.from_numpy(pos.reshape(-1, 9)).to("cuda:0")
            torch.cuda.synchronize()
            emit(kind="wall", call="fr_update_positions device refit",
                 ms=timed(lambda: a.set_positions_device(dev.data_ptr(), n, update="refit")), **common)
            emit(kind="wall", call="fr_update_positions device rebuild",
                 ms=timed(lambda: b.set_positions_device(dev.data_ptr(), n, update="rebuild")), **common)
        emit(kind="wall", call="fr_update_positions host rebuild (fr_set_positions)", ms=timed(lambda: b.set_positions(pos)),
             **common)
        emit(kind="wall", call="fr_rebuild_bvh", ms=[a.rebuild_bvh() for _ in range(6)], **common)
        a.destroy(); b.destroy()

    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        for r in rows:
            f.write(json.dumps(r) + "\n")

    print("\n| scene | tree | amplitude | SAH cost | cost / cost at build | shade_paths ms |")
    print("|---|---|---|---|---|---|")
    built = {}
    for r in rows:
        if r["kind"] != "quality":
            continue
        if r["amplitude"] is None:
            built[r["scene"]] = r["cost"]
        amp = "-" if r["amplitude"] is None else f"{100 * r['amplitude']:g} %"
        ratio = f"{r['cost'] / built[r['scene']]:.2f}" if r["tree"].startswith("host SAH") else "-"
        print(f"| {r['scene']} | {r['tree']} | {amp} | {r['cost']:.2f} | {ratio} | {r['shade_paths_ms']:.3f} |")
    print("\n| scene | call | six calls, ms | median |")
    print("|---|---|---|---|")
    for r in rows:
        if r["kind"] == "wall":
            print(f"| {r['scene']} | {r['call']} | {' '.join(f'{m:.2f}' for m in r['ms'])} | {statistics.median(r['ms']):.2f} |")


if __name__ == "__main__":
    main()
