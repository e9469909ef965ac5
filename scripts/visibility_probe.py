"""Per-model visibility (fr_set_model_visibility, fr_set_model_visibility_enqueue) on the bench workload: 4K, signed
log-polar mask, 4 spp, GI 3, the host-built tree, bunny (and vokselia for k_hide's own time). One context per process:
`--arm X` is one arm (a child of the driver). Arms:
  fps_all, fps_nobox, fps_nobunny   untimed fr_frame alone, with every model visible, the glass box hidden, the bunny
                                    hidden (one synchronous refit before the rounds)
  upd_none, upd_bunny               fr_update_geometry_enqueue (normals recomputed, a sine alternating between 10 % and
                                    5 % of the box diagonal) and fr_geometry_consumed around every untimed fr_frame,
                                    with nothing hidden and with the bunny hidden; in place
  upd_none_ov, upd_bunny_ov         the same with fr_set_geometry_overlap on
  upd_none_p, upd_none_ov_p         upd_none and upd_none_ov on an older library (--lib): the parent's numbers
  idle                              on an idle context, six times each: the time until the call returns and until
                                    fr_synchronize returns, of fr_set_model_visibility_enqueue (the bunny hidden and
                                    shown by turns) and of fr_update_geometry_enqueue with kept normals
  idle_p                            the update of `idle` on the older library
A timed arm is three rounds of 30 warm-up and 60 timed frames (host clock around the loop, the context synchronised
before and after). Without --arm the script is the driver: one child per arm, --reps times, the order reversed every
other time; JSON lines go to --out, tables to stdout. Any failing call ends the script.

--trace-frames N [--scene S] runs N frames with a visibility change enqueued before each (the first model with more
than 1000 triangles hidden and shown by turns) and exits: the run to put under
`rocprofv3 --kernel-trace --stats -- python scripts/visibility_probe.py --trace-frames 40` for k_hide's own time.
Usage: visibility_probe.py [--out FILE] [--reps N] [--arms a,b] [--lib OLDER_LIB]"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
WARMUP, TIMED, ROUNDS = 30, 60, 3
FPS_ARMS = ("fps_all", "fps_nobox", "fps_nobunny")
UPD_ARMS = ("upd_none", "upd_bunny", "upd_none_ov", "upd_bunny_ov")
OLDER_ARMS = ("upd_none_p", "upd_none_ov_p", "idle_p")


def hiding(models, name):
    names = [m[0] for m in models]
    return 0xFFFFFFFF & ~(1 << names.index(name))


def timed_call(t, call):
    t.synchronize()
    t0 = time.perf_counter()
    call()
    t1 = time.perf_counter()
    t.synchronize()
    return (t1 - t0) * 1e3, (time.perf_counter() - t0) * 1e3


def child(arm, scene, trace_frames):
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    import refit_probe as rp  # (make, deform: the configuration; imports torch before libfovrt)
    import torch
    np = rp.np
    older = arm.endswith("_p")
    t = rp.make(scene, 0)
    models = t.models()
    arrays = t.scene_arrays()
    base = arrays["pos"].reshape(-1, 3, 3).copy()
    bbox = np.asarray(arrays["bbox"], np.float32)
    diag = float(np.linalg.norm(bbox[3:] - bbox[:3]))
    n = base.shape[0]
    common = dict(arm=arm, scene=scene, tris=n, lib=os.environ.get("FOVRT_LIB", ""))
    if not older:
        t.enable_model_visibility()
    if trace_frames:
        big = [m[0] for m in models if m[2] > 1000][0]
        for i in range(trace_frames):
            t.set_model_visibility(hiding(models, big) if i % 2 == 0 else 0xFFFFFFFF, enqueue=True)
            t.frame(False)
        t.synchronize()
        t.destroy()
        return
    stream = torch.cuda.current_stream()
    if arm in ("idle", "idle_p"):
        keep = torch.from_numpy(rp.deform(base, 0.05 * diag, bbox).reshape(-1, 9)).to("cuda:0")
        torch.cuda.synchronize()
        t.update_geometry_enqueue(keep, ntris=n)  # (the first enqueue of a context seeds the device's scene box)
        rows = {"update_keep": [timed_call(t, lambda: t.update_geometry_enqueue(keep, ntris=n)) for _ in range(6)]}
        if not older:
            masks = [hiding(models, "bunny"), 0xFFFFFFFF] * 6
            rows["visibility"] = [timed_call(t, lambda m=m: t.set_model_visibility(m, enqueue=True)) for m in masks]
            rows["visibility_hide"] = rows["visibility"][0::2]
            rows["visibility_show"] = rows.pop("visibility")[1::2]
        for k, v in rows.items():
            print(json.dumps(dict(kind="idle", call=k, call_ms=[a for a, _ in v], done_ms=[b for _, b in v], **common)),
                  flush=True)
        torch.cuda.synchronize()
        t.destroy()
        return
    update = arm.startswith("upd")
    if update:
        dev = [torch.from_numpy(rp.deform(base, amp * diag, bbox).reshape(-1, 9)).to("cuda:0") for amp in (0.10, 0.05)]
        torch.cuda.synchronize()
        if "_ov" in arm:
            t.set_geometry_overlap(True)
    hidden = {"fps_nobox": "box", "fps_nobunny": "bunny", "upd_bunny": "bunny", "upd_bunny_ov": "bunny"}.get(arm)
    if hidden:
        t.set_model_visibility(hiding(models, hidden))

    def run(frames):
        for i in range(frames):
            if update:
                t.update_geometry_enqueue(dev[i & 1], ntris=n, normals="recompute")
            t.frame(False)
            if update:
                t.geometry_consumed(stream)

    for r in range(ROUNDS):
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
                              shade_paths_ms=k["shade_paths_ms"] / max(k["frames"], 1), rays=t.ray_count(),
                              sah_cost=t.bvh_sah_cost(), **common)), flush=True)
    if update:
        assert t.geometry_update_status() == (ROUNDS * (WARMUP + TIMED), 0)
    torch.cuda.synchronize()
    t.destroy()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "visibility_probe.jsonl"))
    ap.add_argument("--arm")
    ap.add_argument("--scene", type=int, default=1)
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--arms", default=",".join(FPS_ARMS + UPD_ARMS + ("idle",)))
    ap.add_argument("--lib", help="an older build of the library: adds the arms that end in _p")
    ap.add_argument("--trace-frames", type=int, default=0)
    args = ap.parse_args()
    if args.arm or args.trace_frames:
        return child(args.arm or "trace", args.scene, args.trace_frames)
    arms = tuple(args.arms.split(",")) + (OLDER_ARMS if args.lib else ())
    rows = []
    for rep in range(args.reps):
        for arm in (arms if rep % 2 == 0 else arms[::-1]):
            env = dict(os.environ)
            if arm.endswith("_p"):
                env.update(FOVRT_LIB=os.path.abspath(args.lib), FOVRT_LIB_OLDER="1")
            out = subprocess.run([sys.executable, os.path.abspath(__file__), "--arm", arm, "--scene", str(args.scene)],
                                 env=env, check=True, stdout=subprocess.PIPE, text=True, timeout=300).stdout
            got = [dict(json.loads(line), rep=rep) for line in out.splitlines() if line.startswith("{")]
            for r in got:
                print(json.dumps(r), flush=True)
            rows.extend(got)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        for r in rows:
            f.write(json.dumps(r) + "\n")
    print("\n| arm | fps per round | median | min | max | shade_paths ms, median | active pixels | SAH cost |")
    print("|---|---|---|---|---|---|---|---|")
    for arm in arms:
        sel = [r for r in rows if r["kind"] == "fps" and r["arm"] == arm]
        if not sel:
            continue
        v = [r["fps"] for r in sel]
        print(f"| {arm} | {' '.join(f'{x:.1f}' for x in v)} | {statistics.median(v):.1f} | {min(v):.1f} | {max(v):.1f} | "
              f"{statistics.median(r['shade_paths_ms'] for r in sel):.3f} | {sel[-1]['rays']} | {sel[-1]['sah_cost']:.3f} |")
    print("\n| library | call | the call returns after, ms | the work is done after, ms | median call | median done |")
    print("|---|---|---|---|---|---|")
    for r in rows:
        if r["kind"] == "idle":
            print(f"| {'older' if r['lib'] else 'this'} | {r['call']} | {' '.join(f'{m:.3f}' for m in r['call_ms'])} | "
                  f"{' '.join(f'{m:.3f}' for m in r['done_ms'])} | {statistics.median(r['call_ms']):.3f} | "
                  f"{statistics.median(r['done_ms']):.3f} |")


if __name__ == "__main__":
    main()
