"""The device-triggered rebuild (fr_set_rebuild_policy, fr_rebuild_bvh_enqueue_if) under animation, on
rebuild_enqueue_probe.py's protocol: 4K, signed log-polar mask, 4 spp, GI 3, builder 2, bunny and vokselia,
fr_set_geometry_overlap on, an update enqueued before every untimed fr_frame (normals recomputed). Arms:
  c  fr_rebuild_bvh_enqueue before every eighth frame, under the alternating sine (10 % / 5 % of the box diagonal)
  d  no rebuild at all, same deformation; at the end it prints the SAH cost of its tree when built and refitted over
     either amplitude: the range the ratio is chosen from
  e  fr_set_rebuild_policy(r, 8), same deformation
  f  e under a sine whose amplitude keeps growing (5 % of the diagonal, plus 0.05 % with every frame of the run;
     positions made on the device by torch before every update and handed over with a ready event)
r is not a constant of the script: the driver runs arm d of a scene first and takes r = 1 + 2 (hi / lo - 1), hi and lo
the costs of arm d's tree refitted over the two amplitudes (never below 1.01): twice the swing between the two phases
the bounded deformation alternates between, so the policy pays for no build there whichever phase its first evaluation
adopted, and growth of twice that swing past the baseline does. (The built tree's cost is printed but is not in the
range: the policy's baseline is a refitted tree's, adopted at the first evaluation. 1.25 times the widest of the three
costs, tried first, never built under arm f on either scene.) One context per process: `--arm X --scene S` is one arm (a child of the driver), three rounds of 32
warm-up and 96 timed frames (host clock around the loop, the context synchronised before and after; the live
megakernel time from fr_kernel_timing), then built / skipped from the status calls. Arm `idle` is the idle-context
cost: six times each, the time until the call returns and until fr_synchronize returns, of a conditional call that
builds (the tree refitted over scattered triangles, then back), of one that skips right behind it, and of the
unconditional call; with --lib the unconditional call of an older library as well (arm `idle_p`).
Without --arm the script is the driver: one child per (scene, arm), interleaved, --reps times, the order reversed
every other time; JSON lines go to --out, tables to stdout. Any failing call ends the script.
Usage: rebuild_policy_probe.py [--out FILE] [--reps N] [--arms c,d,e,f,idle] [--lib OLDER_LIB] [scene ...] (default 1 2)"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
WARMUP, TIMED, ROUNDS, EVERY = 32, 96, 3, 8
ARMS = ("c", "d", "e", "f", "idle")
GROW0, GROW = 0.05, 0.0005


def scattered(np, base, diag):
    """Every triangle moved rigidly by its own seeded offset, even ones one way and odd ones the other: a refitted
    tree over it costs many times the built one (the generator of tests/test_cpu_rebuild_policy.py)."""
    off = np.random.default_rng(7).uniform(0.5, 1.5, (base.shape[0], 1, 3)) * (0.3 * diag)
    off *= np.where(np.arange(base.shape[0]) % 2 == 0, -1.0, 1.0)[:, None, None]
    return (base + off.astype(np.float32)).astype(np.float32)


def idle(t, torch, np, base, diag, common, older):
    n = base.shape[0]
    geo = [torch.from_numpy(g.reshape(-1, 9)).to("cuda:0") for g in (scattered(np, base, diag), base)]
    torch.cuda.synchronize()

    def timed(call):
        t.synchronize()
        t0 = time.perf_counter()
        call()
        t1 = time.perf_counter()
        t.synchronize()
        return (t1 - t0) * 1e3, (time.perf_counter() - t0) * 1e3

    rows = {k: [] for k in (("unconditional",) if older else ("build", "skip", "unconditional"))}
    if not older:
        t.rebuild_bvh_enqueue_if(1.25)  # adopts
        for i in range(6):
            t.set_positions_device(geo[i & 1].data_ptr(), n, update="refit")
            rows["build"].append(timed(lambda: t.rebuild_bvh_enqueue_if(1.25)))
            rows["skip"].append(timed(lambda: t.rebuild_bvh_enqueue_if(1.25)))
        ev, sk, _, _ = t.bvh_rebuild_policy_status()
        common = dict(common, evaluated=ev, skipped=sk, built=t.bvh_rebuild_status()[0])  # (13, 7, 6 when all six built)
    for i in range(6):  # (an unconditional build makes the baseline stale: a loop of its own)
        t.set_positions_device(geo[i & 1].data_ptr(), n, update="refit")
        rows["unconditional"].append(timed(t.rebuild_bvh_enqueue))
    for k, v in rows.items():
        print(json.dumps(dict(kind="idle", call=k, call_ms=[a for a, _ in v], done_ms=[b for _, b in v], **common)),
              flush=True)


def child(arm, scene, rounds, ratio):
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    import refit_probe as rp  # (make, deform: the configuration; imports torch before libfovrt)
    import torch
    np = rp.np
    t = rp.make(scene, 2)
    t.set_geometry_overlap(True)
    arrays = t.scene_arrays()
    base = arrays["pos"].reshape(-1, 3, 3).copy()
    bbox = np.asarray(arrays["bbox"], np.float32)
    diag = float(np.linalg.norm(bbox[3:] - bbox[:3]))
    n = base.shape[0]
    common = dict(arm=arm, scene=scene, tris=n, ratio=ratio, lib=os.environ.get("FOVRT_LIB", ""))
    if arm in ("idle", "idle_p"):
        idle(t, torch, np, base, diag, common, arm == "idle_p")
        torch.cuda.synchronize()
        t.destroy()
        return
    dev = [torch.from_numpy(rp.deform(base, amp * diag, bbox).reshape(-1, 9)).to("cuda:0") for amp in (0.10, 0.05)]
    stream = torch.cuda.current_stream()
    if arm == "f":
        rest = torch.from_numpy(base.reshape(-1, 9)).to("cuda:0")
        unit = torch.from_numpy((rp.deform(base, diag, bbox) - base).reshape(-1, 9)).to("cuda:0")  # amplitude 1
        buf = [torch.empty_like(rest), torch.empty_like(rest)]
        ready = [torch.cuda.Event(), torch.cuda.Event()]
    torch.cuda.synchronize()
    cost_built = t.bvh_sah_cost()
    if arm in ("e", "f"):
        t.set_rebuild_policy(ratio, EVERY)
    count = [0]

    def run(frames):
        for i in range(frames):
            if arm == "f":
                k = count[0] & 1
                torch.add(rest, unit, alpha=GROW0 + GROW * count[0], out=buf[k])
                ready[k].record(stream)
                t.update_geometry_enqueue(buf[k], ntris=n, normals="recompute", ready_event=ready[k])
            else:
                t.update_geometry_enqueue(dev[i & 1], ntris=n, normals="recompute")
            if arm == "c" and i % EVERY == 0:
                t.rebuild_bvh_enqueue()
            t.frame(False)
            t.geometry_consumed(stream)
            count[0] += 1

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
    built, failed = t.bvh_rebuild_status()
    ev, sk, last, cost_base = t.bvh_rebuild_policy_status()
    out = dict(kind="verdicts", built=built, failed=failed, evaluated=ev, skipped=sk, last_cost=last, base_cost=cost_base,
               cost_built=cost_built, cost_end=t.bvh_sah_cost(), **common)
    if arm == "d":  # the range the ratio is chosen from: this tree refitted over either amplitude
        for name, x in zip(("cost_10", "cost_05"), dev):
            t.set_positions_device(x.data_ptr(), n, update="refit")
            out[name] = t.bvh_sah_cost()
    print(json.dumps(out), flush=True)
    torch.cuda.synchronize()
    t.destroy()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rebuild_policy_probe.jsonl"))
    ap.add_argument("--arm")
    ap.add_argument("--scene", type=int, default=1)
    ap.add_argument("--rounds", type=int, default=ROUNDS)
    ap.add_argument("--ratio", type=float, default=1.25)
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--arms", default=",".join(ARMS))
    ap.add_argument("--lib", help="an older build of the library: adds arm idle_p, its unconditional call")
    ap.add_argument("scenes", nargs="*", type=int, default=[1, 2])
    args = ap.parse_args()
    if args.arm:
        return child(args.arm, args.scene, args.rounds, args.ratio)
    arms = tuple(args.arms.split(",")) + (("idle_p",) if args.lib else ())
    rows, ratios = [], {}

    def spawn(scene, arm, rep, ratio):
        env = dict(os.environ)
        if arm == "idle_p":
            env.update(FOVRT_LIB=os.path.abspath(args.lib), FOVRT_LIB_OLDER="1")
        out = subprocess.run([sys.executable, os.path.abspath(__file__), "--arm", arm, "--scene", str(scene), "--rounds",
                              str(args.rounds), "--ratio", repr(ratio)], env=env, check=True, stdout=subprocess.PIPE,
                             text=True, timeout=300).stdout
        got = [dict(json.loads(line), rep=rep) for line in out.splitlines() if line.startswith("{")]
        for r in got:
            print(json.dumps(r), flush=True)
        rows.extend(got)
        return got

    for scene in args.scenes:
        first = [r for r in spawn(scene, "d", -1, 1.25) if r["kind"] == "verdicts"][0]  # (not a timed repetition)
        costs = [first["cost_built"], first["cost_10"], first["cost_05"]]
        swing = max(costs[1:]) / min(costs[1:])
        ratios[scene] = max(1.01, 1.0 + 2.0 * (swing - 1.0))
        print(f"scene {scene}: arm d's costs built {costs[0]:.4f}, refitted over 10 % {costs[1]:.4f}, over 5 % "
              f"{costs[2]:.4f}; r = 1 + 2 * ({swing:.4f} - 1) = {ratios[scene]:.4f}", flush=True)
        for rep in range(args.reps):
            for arm in (arms if rep % 2 == 0 else arms[::-1]):
                spawn(scene, arm, rep, ratios[scene])
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        for r in rows:
            f.write(json.dumps(r) + "\n")
    print("\n| scene | arm | r | fps per round | median | min | max | shade_paths ms, median | built | skipped |")
    print("|---|---|---|---|---|---|---|---|---|---|")
    for scene in args.scenes:
        for arm in arms:
            sel = [r for r in rows if r["kind"] == "fps" and r["scene"] == scene and r["arm"] == arm and r["rep"] >= 0]
            if not sel:
                continue
            v = [r["fps"] for r in sel]
            ver = [r for r in rows if r["kind"] == "verdicts" and r["scene"] == scene and r["arm"] == arm and r["rep"] >= 0]
            print(f"| {scene} | {arm} | {ratios[scene]:.3f} | {' '.join(f'{x:.1f}' for x in v)} | {statistics.median(v):.1f} | "
                  f"{min(v):.1f} | {max(v):.1f} | {statistics.median(r['shade_paths_ms'] for r in sel):.3f} | "
                  f"{' '.join(str(r['built']) for r in ver)} | {' '.join(str(r['skipped']) for r in ver)} |")
    print("\n| scene | library | call | the call returns after, ms | the work is done after, ms | median call | median done |")
    print("|---|---|---|---|---|---|---|")
    for r in rows:
        if r["kind"] == "idle":
            print(f"| {r['scene']} | {'older' if r['lib'] else 'this'} | {r['call']} | "
                  f"{' '.join(f'{m:.2f}' for m in r['call_ms'])} | {' '.join(f'{m:.2f}' for m in r['done_ms'])} | "
                  f"{statistics.median(r['call_ms']):.2f} | {statistics.median(r['done_ms']):.2f} |")


if __name__ == "__main__":
    main()
