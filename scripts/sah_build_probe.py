"""The device SAH builder (bvh_builder 2) against the other two, at 4K, per scene (bunny, vokselia):

 (a) wall time of fr_create with builders 0 (host SAH), 1 (device LBVH) and 2 (device SAH);
 (b) wall time of six fr_rebuild_bvh calls in a row with builders 1 and 2;
 (c) the live megakernel time (fr_kernel_timing's shade_paths_ms over 20 pipelined frames after 5) under the sine
     deformation of refit_probe.py at 2 % and 10 % of the scene-box diagonal, over three trees of the same
     positions: builder 2 rebuilt, builder 1 rebuilt, builder 0 refitted; and the same run twice over the untouched
     builder 0 and builder 2 trees, for the run-to-run spread and the "equal by construction" check.

Writes one JSON line per measurement to --out (default profiles/sah_build_probe.jsonl) and prints markdown tables.
Usage: sah_build_probe.py [--out FILE] [scene ...] (default 1 2)."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import refit_probe as rp  # noqa: E402  (make, deform, trace_ms: the configuration of "Refit against rebuild")

AMPLITUDES = (0.02, 0.10)
BUILDERS = {0: "host SAH", 1: "device LBVH", 2: "device SAH"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sah_build_probe.jsonl"))
    ap.add_argument("scenes", nargs="*", type=int, default=[1, 2])
    args = ap.parse_args()
    rows = []

    def emit(**kw):
        rows.append(kw)
        print(json.dumps(kw), flush=True)

    for scene in args.scenes:
        rp.make(scene, 0).destroy()  # the process's first context pays the runtime's start-up
        t, create = {}, {}
        for b in BUILDERS:
            t0 = time.perf_counter()
            t[b] = rp.make(scene, b)
            create[b] = (time.perf_counter() - t0) * 1e3
        arrays = t[0].scene_arrays()
        base = arrays["pos"].reshape(-1, 3, 3).copy()
        bbox = rp.np.asarray(arrays["bbox"], rp.np.float32)
        diag = float(rp.np.linalg.norm(bbox[3:] - bbox[:3]))
        common = dict(scene=scene, tris=base.shape[0])
        for b in BUILDERS:
            emit(kind="create", builder=b, ms=create[b], nodes=t[b].scene_arrays()["bvh_nodes"],
                 cost=t[b].bvh_sah_cost(), **common)
        # the same run twice, and the two SAH trees against each other
        for b in (0, 2):
            emit(kind="trace", tree=f"{BUILDERS[b]}, untouched", amplitude=None,
                 shade_paths_ms=[rp.trace_ms(t[b]) for _ in range(2)], **common)
        for amp in AMPLITUDES:
            pos = rp.deform(base, amp * diag, bbox)
            t[0].set_positions(pos, update="refit")
            t[1].set_positions(pos)
            t[2].set_positions(pos)
            for b, how in ((2, "rebuilt"), (1, "rebuilt"), (0, "refitted")):
                emit(kind="trace", tree=f"{BUILDERS[b]}, {how}", amplitude=amp, cost=t[b].bvh_sah_cost(),
                     shade_paths_ms=[rp.trace_ms(t[b])], **common)
        for b in (1, 2):
            emit(kind="rebuild", builder=b, ms=[t[b].rebuild_bvh() for _ in range(6)], **common)
        for x in t.values():
            x.destroy()

    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        for r in rows:
            f.write(json.dumps(r) + "\n")

    print("\n| scene | builder | fr_create ms | nodes | SAH cost |")
    print("|---|---|---|---|---|")
    for r in rows:
        if r["kind"] == "create":
            print(f"| {r['scene']} | {BUILDERS[r['builder']]} | {r['ms']:.0f} | {r['nodes']} | {r['cost']:.2f} |")
    print("\n| scene | builder | fr_rebuild_bvh, six calls, ms | median |")
    print("|---|---|---|---|")
    for r in rows:
        if r["kind"] == "rebuild":
            print(f"| {r['scene']} | {BUILDERS[r['builder']]} | {' '.join(f'{m:.2f}' for m in r['ms'])} | "
                  f"{statistics.median(r['ms']):.2f} |")
    print("\n| scene | tree | amplitude | SAH cost | shade_paths ms |")
    print("|---|---|---|---|---|")
    for r in rows:
        if r["kind"] == "trace":
            amp = "-" if r["amplitude"] is None else f"{100 * r['amplitude']:g} %"
            cost = f"{r['cost']:.2f}" if "cost" in r else "-"
            print(f"| {r['scene']} | {r['tree']} | {amp} | {cost} | {' '.join(f'{m:.3f}' for m in r['shade_paths_ms'])} |")


if __name__ == "__main__":
    main()
