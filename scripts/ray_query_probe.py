"""Ray queries measured on the bench workload (bunny 4K, 4 spp, GI 3, signed log-polar mask).

Query throughput (arm T): the synchronous device form of fr_trace_rays over
  raster    the frame's W x H camera rays in raster order, closest hit
  shuffled  the same rays in a seeded random order
  shadow    transmittance rays from the G-buffer's hit points towards the light's centre
each timed by a host clock around the call (which ends in a synchronise of the context stream), 3 warm-up calls and
10 timed ones; beside them fr_geometry_launch's own time over the same camera rays (its events), the only other
kernel that traces them (it also writes five images: a reference point, not a bar). Arm G is that launch alone on an
older build (--lib), the parent commit's; arm Tp is arm T's three sets on that build. On this build arm T goes on with
  surface           the raster rays answered as 80-byte fr_ray_surface records (two kernels)
  masked_all        raster, closest hit, every model's bit set in every mask
  masked_no_ground  the same with model 0 left out
  shadow_masked_all the shadow set, every model's bit set
and arm S is the surface query alone, a few calls: the process to take a kernel trace of.

Pipelined frame rate: untimed fr_frame in a loop, 30 warm-up frames and 120 timed ones per round (host clock, the
context synchronised before and after), throughput mode, then latency mode.
  0   no queries           0b  the same again (the A/A spread of this session)
  Q   a 65,536-ray fr_trace_rays_enqueue before every frame (the first rays of the raster set)
  p   no queries, on the older build (--lib)
Every arm is a process of its own; the arms alternate over --reps repetitions, the order reversed every other one.
Writes one JSON line per measurement to --out (default profiles/ray_queries.jsonl) and prints markdown tables.
Usage: ray_query_probe.py [--lib OLDER.so] [--out FILE] [--width W --height H] [--reps N] [--rounds N] [--arms ...]"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, os.path.join(ROOT, "foveated-rendering-using-ray-tracing_amd"))

ASSET_FILES = ("CedarCity.hdr", "grid.ppm", "bunny/bunny.PPM", "vokselia_spawn/vokselia_spawn.png")
WARMUP, TIMED = 30, 120
QUERY_RAYS = 65536


def tracer(fovrt, W, H):
    have = all(os.path.exists(os.path.join(fovrt.DEFAULT_ASSET_DIR, p)) for p in ASSET_FILES)
    t = fovrt.PathTracer(fovrt.Config(width=W, height=H, scene=fovrt.SCENE_BUNNY, mask_mode=fovrt.MASK_LOGPOLAR_SIGNED,
                                      spp=4, diffuse_max_depth=3, texture_mode=0 if have else 1))
    t.initialize()
    t.update_optix_variables(fovrt.Camera.preset(fovrt.SCENE_BUNNY, W, H))
    return t


def camera_rays(torch, fovrt, W, H):
    """The G-buffer's camera rays as fr_ray rows on the device (fp32; near = inv_vp (ndc, -1, 1), d = normalize(near /
    w - eye), tmin 1e-3, tmax inf): the directions the frame traces, to rounding."""
    uni = fovrt.Camera.preset(fovrt.SCENE_BUNNY, W, H).uniforms(W, H)
    m = torch.tensor(list(uni.inv_vp), dtype=torch.float32, device="cuda:0").reshape(4, 4)
    eye = torch.tensor(list(uni.eye), dtype=torch.float32, device="cuda:0")
    x = (torch.arange(W, dtype=torch.float32, device="cuda:0") / W * 2 - 1)[None, :].expand(H, W)
    y = (torch.arange(H, dtype=torch.float32, device="cuda:0") / H * 2 - 1)[:, None].expand(H, W)
    v = torch.stack([x, y, -torch.ones_like(x), torch.ones_like(x)], -1) @ m.T
    d = v[..., :3] / v[..., 3:4] - eye
    d = d / d.norm(dim=-1, keepdim=True)
    rays = torch.empty((H * W, 8), dtype=torch.float32, device="cuda:0")
    rays[:, 0:3], rays[:, 3], rays[:, 4:7], rays[:, 7] = eye, 1e-3, d.reshape(-1, 3), float("inf")
    return rays


def timed_calls(fn, warm=3, reps=10):
    for _ in range(warm):
        fn()
    ms = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ms.append((time.perf_counter() - t0) * 1e3)
    return ms


def child(arm, W, H, rounds):
    import torch  # before libfovrt: one HIP runtime in the process
    import fovrt
    t = tracer(fovrt, W, H)
    common = dict(arm=arm, width=W, height=H, lib="older" if os.environ.get("FOVRT_LIB") else "built")
    if arm == "S":  # the surface query alone, a few calls: the process a kernel trace is taken of
        rays = camera_rays(torch, fovrt, W, H)
        n = rays.shape[0]
        out = torch.empty((n, 20), dtype=torch.float32, device="cuda:0")
        torch.cuda.synchronize()
        ms = timed_calls(lambda: t.trace_rays(rays, "surface", out=out, n=n))
        print(json.dumps(dict(kind="query", set="surface", rays=n, ms=ms, **common)), flush=True)
    elif arm in ("T", "Tp", "G"):
        g = [t.geometry_launch() for _ in range(13)][3:]
        print(json.dumps(dict(kind="geometry_launch", ms=g, rays=W * H, **common)), flush=True)
        if arm in ("T", "Tp"):
            rays = camera_rays(torch, fovrt, W, H)
            n = rays.shape[0]
            out = torch.empty((n, 4), dtype=torch.float32, device="cuda:0")
            shuffled = rays[torch.randperm(n, generator=torch.Generator().manual_seed(1)).to("cuda:0")].contiguous()
            TN = fovrt.TextureName
            t.geometry_launch()
            hit = torch.from_numpy(t.read(TN.GCLASS).reshape(-1) != 3).to("cuda:0")
            p = torch.from_numpy(t.read(TN.POSITION).reshape(-1, 4)[:, :3].copy()).to("cuda:0")[hit]
            L = np.asarray(t.scene_arrays()["light"], np.float64)
            c = torch.tensor(L[0:3] + 0.5 * L[3:6] + 0.5 * L[6:9], dtype=torch.float32, device="cuda:0")
            v = c - p
            dist = v.norm(dim=-1)
            shadow = torch.empty((p.shape[0], 8), dtype=torch.float32, device="cuda:0")
            shadow[:, 0:3], shadow[:, 3], shadow[:, 4:7], shadow[:, 7] = p, 1e-3, v / dist[:, None], dist
            sout = torch.empty(p.shape[0], dtype=torch.float32, device="cuda:0")
            torch.cuda.synchronize()
            for name, r, kind, o in (("raster", rays, "closest", out), ("shuffled", shuffled, "closest", out),
                                     ("shadow", shadow, "transmittance", sout)):
                k = r.shape[0]
                ms = timed_calls(lambda: t.trace_rays(r, kind, out=o, n=k))
                print(json.dumps(dict(kind="query", set=name, rays=k, ms=ms,
                                      mrays_per_s=k / (statistics.median(ms) * 1e-3) / 1e6, **common)), flush=True)
            hits = out.cpu().numpy().view(fovrt.RAY_HIT_DTYPE).reshape(-1)["prim"] >= 0
            print(json.dumps(dict(kind="check", shuffled_hit_share=float(hits.mean()),
                                  gbuffer_hit_share=float(hit.float().mean()),
                                  shadow_mean=float(sout.mean()), **common)), flush=True)
            if arm == "T":  # the second part's kinds, on this build only
                surf = torch.empty((n, 20), dtype=torch.float32, device="cuda:0")
                nm = len(t.models())
                every = torch.full((n,), (1 << nm) - 1, dtype=torch.int32, device="cuda:0")
                no_ground = torch.full((n,), ((1 << nm) - 1) & ~1, dtype=torch.int32, device="cuda:0")
                every_s = every[:shadow.shape[0]].contiguous()
                torch.cuda.synchronize()
                for name, rr, kind, o, m in (("surface", rays, "surface", surf, None),
                                             ("masked_all", rays, "closest", out, every),
                                             ("masked_no_ground", rays, "closest", out, no_ground),
                                             ("shadow_masked_all", shadow, "transmittance", sout, every_s)):
                    k = rr.shape[0]
                    ms = timed_calls(lambda: t.trace_rays(rr, kind, out=o, n=k, masks=m))
                    print(json.dumps(dict(kind="query", set=name, rays=k, ms=ms,
                                          mrays_per_s=k / (statistics.median(ms) * 1e-3) / 1e6, **common)), flush=True)
                    if kind == "closest":
                        h = out.cpu().numpy().view(fovrt.RAY_HIT_DTYPE).reshape(-1)["prim"] >= 0
                        print(json.dumps(dict(kind="check", set=name, hit_share=float(h.mean()), **common)), flush=True)
    else:
        rays = out = None
        if arm == "Q":
            rays = camera_rays(torch, fovrt, W, H)[:QUERY_RAYS].contiguous()
            out = torch.empty((QUERY_RAYS, 4), dtype=torch.float32, device="cuda:0")
            torch.cuda.synchronize()
        for mode in ("throughput", "latency"):
            t.set_pipeline_mode(fovrt.PIPELINE_LATENCY if mode == "latency" else fovrt.PIPELINE_THROUGHPUT)
            for r in range(rounds):
                for frames in (WARMUP, TIMED):
                    t.synchronize()
                    t0 = time.perf_counter()
                    for _ in range(frames):
                        if arm == "Q":
                            t.trace_rays_enqueue(rays, out, n=QUERY_RAYS)
                        t.frame(timing=False)
                    t.synchronize()
                    dt = time.perf_counter() - t0
                print(json.dumps(dict(kind="fps", mode=mode, round=r, fps=TIMED / dt, **common)), flush=True)
    torch.cuda.synchronize()
    t.destroy()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ray_queries.jsonl"))
    ap.add_argument("--arm")
    ap.add_argument("--width", type=int, default=3840)
    ap.add_argument("--height", type=int, default=2160)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=4)
    ap.add_argument("--arms", default="T,0,0b,Q")
    ap.add_argument("--lib", help="an older build of the library (the parent commit's): adds arms G and p over it")
    args = ap.parse_args()
    if args.arm:
        return child(args.arm, args.width, args.height, args.rounds)
    arms = tuple(args.arms.split(","))
    arms += tuple(a for a in ("G", "p", "Tp") if args.lib and a not in arms)
    rows = []
    for rep in range(args.reps):
        for arm in (arms if rep % 2 == 0 else arms[::-1]):
            if arm in ("T", "Tp", "G", "S") and rep >= 2:
                continue  # (two processes of each are enough: their calls repeat inside)
            env = dict(os.environ)
            if arm in ("G", "p", "Tp"):
                env.update(FOVRT_LIB=os.path.abspath(args.lib), FOVRT_LIB_OLDER="1")
            res = subprocess.run([sys.executable, os.path.abspath(__file__), "--arm", arm, "--width", str(args.width),
                                  "--height", str(args.height), "--rounds", str(args.rounds)], env=env, check=True,
                                 stdout=subprocess.PIPE, text=True, timeout=400).stdout
            for line in res.splitlines():
                if line.startswith("{"):
                    rows.append(dict(json.loads(line), rep=rep))
                    print(line, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        for r in rows:
            f.write(json.dumps(r) + "\n")
    med = statistics.median
    print("\n| measurement | rays | ms per call: median (min .. max) | Mrays/s at the median |")
    print("|---|---|---|---|")
    for r in rows:
        if r["kind"] in ("query", "geometry_launch"):
            name = r.get("set", "fr_geometry_launch") + f" (arm {r['arm']}, rep {r['rep']})"
            print(f"| {name} | {r['rays']} | {med(r['ms']):.3f} ({min(r['ms']):.3f} .. {max(r['ms']):.3f}) | "
                  f"{r['rays'] / (med(r['ms']) * 1e-3) / 1e6:.0f} |")
    print("\n| mode | arm | fps per process (median of its rounds) | median | min | max |")
    print("|---|---|---|---|---|---|")
    for mode in ("throughput", "latency"):
        for arm in arms:
            per = {}
            for r in rows:
                if r["kind"] == "fps" and r["mode"] == mode and r["arm"] == arm:
                    per.setdefault(r["rep"], []).append(r["fps"])
            v = [med(x) for x in per.values()]
            if v:
                print(f"| {mode} | {arm} | {' '.join(f'{x:.1f}' for x in v)} | {med(v):.1f} | {min(v):.1f} | {max(v):.1f} |")


if __name__ == "__main__":
    main()
