"""A rebuild every eighth frame under a deformation enqueued before every frame (fr_rebuild_bvh_enqueue against the
synchronous fr_rebuild_bvh): the configuration of "Refit against rebuild" (4K, signed log-polar mask, 4 spp, GI 3),
builder 2, bunny and vokselia. The sine deformation of refit_probe.py alternates between 10 % and 5 % of the
scene-box diagonal through fr_update_geometry_enqueue (normals recomputed) before every untimed fr_frame. Arms:
  a  fr_rebuild_bvh (synchronous) before every eighth frame       (also with another library: --lib, arm "p")
  b  fr_rebuild_bvh_enqueue, updates and rebuilds in place
  c  b with fr_set_geometry_overlap on
  d  no rebuild at all
One context per process: `--arm X --scene S` is one arm (a child of the driver), three rounds of 32 warm-up and 96
timed frames (host clock around the loop, the context synchronised before and after; the live megakernel time of
the timed frames from fr_kernel_timing), then the build alone on the idle context: six times the wall time of
enqueue + fr_synchronize (arms b, c) or of fr_rebuild_bvh (arm a). Without --arm the script is the driver: it
starts one child process per (scene, arm), the arms interleaved, --reps times, the order reversed every other time,
and appends every child's JSON lines to --out (default profiles/rebuild_enqueue_probe.jsonl), then prints tables.
Any failing call ends the script.
Usage: rebuild_enqueue_probe.py [--out FILE] [--reps N] [--arms a,b,c,d] [--lib OLDER_LIB] [scene ...] (default 1 2)"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
WARMUP, TIMED, ROUNDS, EVERY = 32, 96, 3, 8
ARMS = ("a", "b", "c", "d")


def child(arm, scene, rounds):
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    import refit_probe as rp  # (make, deform: the configuration; imports torch before libfovrt)
    import torch
    np = rp.np
    t = rp.make(scene, 2)
    if arm == "c":
        t.set_geometry_overlap(True)
    arrays = t.scene_arrays()
    base = arrays["pos"].reshape(-1, 3, 3).copy()
    bbox = np.asarray(arrays["bbox"], np.float32)
    diag = float(np.linalg.norm(bbox[3:] - bbox[:3]))
    n = base.shape[0]
    dev = [torch.from_numpy(rp.deform(base, amp * diag, bbox).reshape(-1, 9)).to("cuda:0") for amp in (0.10, 0.05)]
    torch.cuda.synchronize()
    stream = torch.cuda.current_stream()
    enq = arm in ("b", "c")

    def run(frames):
        for i in range(frames):
            t.update_geometry_enqueue(dev[i & 1], ntris=n, normals="recompute")
            if i % EVERY == 0:
                if enq:
                    t.rebuild_bvh_enqueue()
                elif arm in ("a", "p"):
                    t.rebuild_bvh()
            t.frame(False)
            t.geometry_consumed(stream)

    common = dict(arm=arm, scene=scene, tris=n, lib=os.environ.get("FOVRT_LIB", ""))
    for r in range(rounds):
        run(WARMUP)
        t.synchronize()
        t.kernel_timing(True)
        t0 = time.perf_counter()
        run(TIMED)
        t.synchronize()
        dt = time.perf_counter() - t0
        k = t.kernel_times()
        t.kernel_timing(False)
        print(json.dumps(dict(kind="fps", round=r, frames=TIMED, fps=TIMED / dt, ms_per_frame=1e3 * dt / TIMED,
                              shade_paths_ms=k["shade_paths_ms"] / max(k["frames"], 1), **common)), flush=True)
    if arm != "d":
        ms = []
        for _ in range(6):
            t.synchronize()
            t0 = time.perf_counter()
            if enq:
                t.rebuild_bvh_enqueue()
                t1 = time.perf_counter()
                t.synchronize()
            else:
                t.rebuild_bvh()
                t1 = time.perf_counter()
            ms.append(dict(call=(t1 - t0) * 1e3, done=(time.perf_counter() - t0) * 1e3))
        print(json.dumps(dict(kind="build", call_ms=[m["call"] for m in ms], done_ms=[m["done"] for m in ms],
                              nodes=t.scene_arrays()["bvh_nodes"], cost=t.bvh_sah_cost(), **common)), flush=True)
    if enq:
        built, failed = t.bvh_rebuild_status()
        assert failed == 0 and built == rounds * (WARMUP // EVERY + TIMED // EVERY) + 6, (built, failed)
    torch.cuda.synchronize()
    t.destroy()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rebuild_enqueue_probe.jsonl"))
    ap.add_argument("--arm")
    ap.add_argument("--scene", type=int, default=1)
    ap.add_argument("--rounds", type=int, default=ROUNDS)
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--arms", default=",".join(ARMS))
    ap.add_argument("--lib", help="an older build of the library: adds arm p, arm a over it")
    ap.add_argument("scenes", nargs="*", type=int, default=[1, 2])
    args = ap.parse_args()
    if args.arm:
        return child(args.arm, args.scene, args.rounds)
    arms = tuple(args.arms.split(",")) + (("p",) if args.lib else ())
    rows = []
    for scene in args.scenes:
        for rep in range(args.reps):
            for arm in (arms if rep % 2 == 0 else arms[::-1]):
                env = dict(os.environ)
                if arm == "p":
                    env.update(FOVRT_LIB=os.path.abspath(args.lib), FOVRT_LIB_OLDER="1")
                out = subprocess.run([sys.executable, os.path.abspath(__file__), "--arm", arm, "--scene", str(scene),
                                      "--rounds", str(args.rounds)], env=env, check=True, stdout=subprocess.PIPE,
                                     text=True, timeout=300).stdout
                for line in out.splitlines():
                    if line.startswith("{"):
                        rows.append(dict(json.loads(line), rep=rep))
                        print(line, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        for r in rows:
            f.write(json.dumps(r) + "\n")
    print("\n| scene | arm | fps per round | median | min | max | shade_paths ms, median |")
    print("|---|---|---|---|---|---|---|")
    for scene in args.scenes:
        for arm in arms:
            sel = [r for r in rows if r["kind"] == "fps" and r["scene"] == scene and r["arm"] == arm]
            v = [r["fps"] for r in sel]
            print(f"| {scene} | {arm} | {' '.join(f'{x:.1f}' for x in v)} | {statistics.median(v):.1f} | {min(v):.1f} | "
                  f"{max(v):.1f} | {statistics.median(r['shade_paths_ms'] for r in sel):.3f} |")
    print("\n| scene | arm | the call returns after, ms | the build is done after, ms | median done |")
    print("|---|---|---|---|---|")
    for r in rows:
        if r["kind"] == "build":
            print(f"| {r['scene']} | {r['arm']} | {' '.join(f'{m:.2f}' for m in r['call_ms'])} | "
                  f"{' '.join(f'{m:.2f}' for m in r['done_ms'])} | {statistics.median(r['done_ms']):.2f} |")


if __name__ == "__main__":
    main()
