"""Call sequences over the frame path's deferred and retained state (pure Python, no device).

The frame path avoids work with host flags: an image is owed and written on demand (jfa_coord_owed, extra.owed), or
retained state still describes a buffer (sib_prefix_fresh / jfa_final, jfa_force / jfa_reuse, hvalid_fresh, lp_gaze /
lp_mode / fov_dirty, compacted / mask_dirty). Every call that writes a buffer or changes what the next launch sees has
to keep all of them right. The cases here are sequences prefix, disturber, observer of named steps; the GPU test
(test_gpu_state_sequences.py) makes the same calls on a default context and on one created with every shortcut
switched off, and holds what the observer read to bit equality. The CPU test (test_cpu_state_sequences.py) holds the
tables themselves: deterministic, complete, and the walks meeting the pairs they must meet.

A step is Step(name, fn): fn(fovrt, t, env) makes its calls on the tracer it is given. env (Env) is made anew, from
the same arguments, for every arm of a case: the camera list, the gaze list, a seeded rng for written patterns, the
snapshots, and what the steps read (env.obs). Reads go through fr_read_buffer directly (raw_read): PathTracer.read()
takes a view first, a view of EXTRA makes the context eager for good and a view of a JFA output clears
sib_prefix_fresh, so read() would erase the state under test. view() appears only as a disturber.

Written patterns stay inside what the kernels trust of a buffer: WEIGHT (its .xy index the history), MASK, DEPTH and
JFA_COORD (seed coordinates) are written with their own bytes read back; a pattern SHADING is a sparse image (alpha 1
on about 5 % of the pixels, 0 elsewhere), a pattern JFA_COLOR keeps its own alpha."""
import numpy as np

SIZES = [(96, 64), (100, 70)]  # whole 16x16 blocks; ragged on both axes, a partial last word of the JFA seed bitmap
SCENE, MASK_MODE, SPP, DIFFUSE_MAX_DEPTH, SIBSON_MODE = 1, 4, 1, 1, 0  # the bunny, signed log-polar, the run form
KNOBS = ("FOVRT_JFA_LAZY_OUTPUTS", "FOVRT_EXTRA_LAZY", "FOVRT_JFA_REUSE", "FOVRT_EARLY_SETUP")  # "0": shortcut off
N_CAMERAS = N_GAZES = 64
MOVED_MODEL, MOVED_BY = "earth", (0.0, 0.6, 0.0)  # its top leaves the scene box (y <= 1.5)
HIDDEN_MODEL = "box"


class Step:
    def __init__(self, name, fn, before_prefix=None):
        self.name, self.fn, self.before_prefix = name, fn, before_prefix

    def __repr__(self):
        return self.name


class Env:
    """What the steps of one run on one tracer share. cameras: fr_camera uniforms of a panning camera; gazes: window
    coordinates; base_snap: the tracer's snapshot right after fr_create (the prefixes start from it); rest: the
    scene's positions as created, (ntris, 9); models: PathTracer.models()."""

    def __init__(self, cameras, gazes, seed, base_snap, rest, models):
        self.cameras, self.gazes = cameras, gazes
        # where the pan and the gazes start depends on the seed: the images a case leaves in a shared context are
        # not the ones the next case owes
        self.cam_i, self.gaze_i = seed % N_CAMERAS, seed // N_CAMERAS % N_GAZES
        self.rng = np.random.default_rng(seed)
        self.base_snap, self.rest, self.models = base_snap, rest, models
        self.snap_earlier = None    # taken one frame before the prefix ended
        self.sibson_before = None   # SIBSON as a restore disturber found it
        self.rays = self.ray_ref = None
        self.geometry_at_rest = True
        self.obs = []               # (step name, {buffer name: array}) in call order

    def next_view(self, t):
        """The next camera of the pan, then the next gaze (fr_set_camera centres the gaze)."""
        t.set_camera_uniforms(self.cameras[self.cam_i % len(self.cameras)])
        self.cam_i += 1
        self.next_gaze(t)

    def next_gaze(self, t):
        t.set_gaze(*self.gazes[self.gaze_i % len(self.gazes)])
        self.gaze_i += 1


def gaze_list(W, H):
    """N_GAZES window positions inside the screen (set_gaze scales a windowed cursor's y by 1.25)."""
    r = np.random.default_rng(W * 1000 + H).random((N_GAZES, 2))
    return [(float((0.1 + 0.8 * a) * W), float((0.1 + 0.8 * b) * H / 1.25)) for a, b in r]


def camera_list(fovrt, W, H):
    """N_CAMERAS uniforms of the bunny preset panning (each one's previous pose is the one before it)."""
    cam = fovrt.Camera.preset(SCENE, W, H)
    out = []
    for _ in range(N_CAMERAS):
        cam.setPrevState()
        cam.lookAt(np.asarray(cam.target) + np.array([0.01, 0.005, 0.0], np.float32))
        out.append(cam.uniforms(W, H))
    return out


def ray_batch(fovrt):
    """A few rays from the preset eye into the scene (RAY_DTYPE rows: origin, tmin, dir, tmax); two of them miss."""
    eye = np.array([0.5, 2.4, 4.9], np.float32)
    to = np.array([[-0.2, 0.92, 0.46], [-1.5, 0.8, 1.2], [0.0, 1.0, 0.0], [-3.5, 0.7, 1.2], [3.0, -0.05, 2.0],
                   [0.5, 30.0, 4.9], [40.0, 9.0, 4.9]], np.float32)
    d = to - eye
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    rays = np.zeros((len(to), 8), np.float32)
    rays[:, 0:3], rays[:, 3], rays[:, 4:7], rays[:, 7] = eye, 1e-3, d, np.inf
    return rays


def moved_positions(rest, models):
    """The scene's positions with MOVED_MODEL translated by MOVED_BY."""
    first, n = next((f, c) for name, f, c in models if name == MOVED_MODEL)
    out = np.array(rest, np.float32).reshape(-1, 3, 3).copy()
    out[first:first + n] += np.asarray(MOVED_BY, np.float32)
    return out.reshape(-1, 9)


def raw_read(fovrt, t, name):
    """fr_read_buffer without the view PathTracer.read() takes first."""
    buf = getattr(fovrt.TextureName, name)
    W, H = t.width, t.height
    out = np.empty((H, W), np.uint8) if name == "MASK" else np.empty((H, W, 4), np.float32)
    t._check(fovrt._lib.fr_read_buffer(t._ctx, int(buf), out.ctypes.data, out.nbytes))
    return out


def observe(fovrt, t, env, step_name, names, extra=None):
    got = {n: raw_read(fovrt, t, n) for n in names}
    if extra:
        got.update(extra)
    env.obs.append((step_name, got))


# ---------------------------------------------------------------------------------------------------------------
# Prefixes: the states to start from. Each begins with `reset`, which brings a context that ran earlier cases back
# to where fr_create left it (as far as a caller can): one shard, both chains, throughput mode, every model visible
# and at rest, and the snapshot taken right after fr_create restored (history, depth, atlases, frame counter, camera,
# gaze, mask mode; a restore forces the next JumpFlooding and drops the mask cache and the validity bits). The two
# images that are written on demand are then overwritten: a context runs many cases, and what an earlier case left
# in JFA_COORD or EXTRA could be, or resemble, the image this case owes, so that a read of the unwritten buffer
# would pass for the written one. What such a read finds now is one valid seed coordinate in every texel of
# JFA_COORD (safe for every kernel that takes seeds from it) and a constant EXTRA.
# ---------------------------------------------------------------------------------------------------------------
def reset(fovrt, t, env):
    W, H = t.width, t.height
    t.set_shard(0, 1)
    t.set_recon_chains(3)
    t.set_pipeline_mode(fovrt.PIPELINE_THROUGHPUT)
    if getattr(t, "_seq_hidden", False):
        t.set_model_visibility(fovrt.FR_VISIBLE_ALL)
        t._seq_hidden = False
    if getattr(t, "_seq_moved", False):
        t.set_positions(env.rest, update="refit")
        t._seq_moved = False
    t.restore(env.base_snap)
    t.set_mask_mode(MASK_MODE)
    stale = np.empty((H, W, 4), np.float32)
    stale[:] = (0.5 / W, 0.5 / H, 0.0, 1.0)
    t.write(fovrt.TextureName.JFA_COORD, stale)
    t.write(fovrt.TextureName.EXTRA, np.full((H, W, 4), 0.125, np.float32))


def _prefix_stage_calls(fovrt, t, env):
    TN = fovrt.TextureName
    reset(fovrt, t, env)
    env.next_view(t)
    env.snap_earlier = t.snapshot()
    t.geometry_launch()
    t.sampling_launch()
    t.optimize_launch()
    t.shading_launch()
    fovrt.JumpFlooding(t).render(TN.SHADING)
    fovrt.SibsonInterpolation(t).render()
    fovrt.PullPushInterpolation(t).render(TN.SHADING)
    fovrt.ATrous(t).render(1, TN.POSITION, TN.NORMAL, TN.PULLPUSH)


def _prefix_frames(mode, timing):
    def run(fovrt, t, env):
        reset(fovrt, t, env)
        t.set_pipeline_mode(mode)
        for k in range(3):
            env.next_view(t)
            if k == 2:
                env.snap_earlier = t.snapshot()
            t.frame(timing=timing)
    return run


PREFIXES = [
    Step("stage_calls", _prefix_stage_calls),                  # JFA_COORD and EXTRA owed, the prefix sums fresh
    Step("frames_throughput", _prefix_frames(0, False)),
    Step("frames_latency", _prefix_frames(1, False)),          # (PIPELINE_LATENCY: the validity bits are fresh)
    Step("frames_timed", _prefix_frames(0, True)),
]
MAIN_PREFIXES = ("stage_calls", "frames_throughput")


# ---------------------------------------------------------------------------------------------------------------
# Disturbers: calls that may invalidate something.
# ---------------------------------------------------------------------------------------------------------------
def _nothing(fovrt, t, env):
    pass


def _snapshot_restore(fovrt, t, env):
    env.sibson_before = raw_read(fovrt, t, "SIBSON")
    t.restore(t.snapshot())


def _restore_earlier(fovrt, t, env):
    env.sibson_before = raw_read(fovrt, t, "SIBSON")
    t.restore(env.snap_earlier)


def _write_own(name):
    def run(fovrt, t, env):
        t.write(getattr(fovrt.TextureName, name), raw_read(fovrt, t, name))
    return run


def _write_pattern(name):
    def run(fovrt, t, env):
        W, H = t.width, t.height
        img = env.rng.random((H, W, 4), dtype=np.float32)
        if name == "SHADING":  # a sparse image: seeds where alpha is 1
            seeds = env.rng.random((H, W)) < 0.05
            img[..., 3] = seeds
            img[~seeds, :3] = 0.0
        elif name == "JFA_COLOR":  # its own alpha: the seeds' flags stay
            img[..., 3] = raw_read(fovrt, t, name)[..., 3]
        elif name == "HISTORY_CACHE":  # part of the history invalid
            img[..., 3] = env.rng.random((H, W)) < 0.7
        t.write(getattr(fovrt.TextureName, name), img)
    return run


def _view(name):
    def run(fovrt, t, env):
        t.view(getattr(fovrt.TextureName, name))
        if name == "EXTRA":
            t._seq_spoiled = True  # every sampling writes EXTRA from now on: the test replaces the context
    return run


def _set_gaze(fovrt, t, env):
    env.next_gaze(t)


def _next_camera(fovrt, t, env):
    t.set_camera_uniforms(env.cameras[env.cam_i % len(env.cameras)])
    env.cam_i += 1


def _mask_mode_0(fovrt, t, env):
    t.set_mask_mode(fovrt.MASK_SALIENCY)


def _mask_mode_5(fovrt, t, env):
    t.set_mask_mode(fovrt.MASK_ECCENTRIC)
    t.set_foveation(radius_px=0.2 * t.width)


def _mask_mode_6(fovrt, t, env):
    W, H = t.width, t.height
    t.enable_sampling_mask(True)
    y, x = np.mgrid[0:H, 0:W]
    t.set_sampling_mask((((x // 3 + y // 2) % 4 == 0) | ((x - W // 3) ** 2 + (y - H // 2) ** 2 < 100)).astype(np.uint8))
    t.set_mask_mode(fovrt.MASK_CALLER)


def _move_model(fovrt, t, env):
    t.set_positions(moved_positions(env.rest, env.models), update="refit")
    t._seq_moved = True
    env.geometry_at_rest = False


def _hide_model(fovrt, t, env):
    t.enable_model_visibility(True)
    names = [m[0] for m in env.models]
    t.set_model_visibility([n for n in names if n != HIDDEN_MODEL])
    t._seq_hidden = True
    env.geometry_at_rest = False


def _recon_chains(fovrt, t, env):
    t.set_recon_chains(2)
    env.next_view(t)
    t.frame(timing=False)  # no JumpFlooding in it: what the last one retained and owes stays
    t.set_recon_chains(3)


def _shard_and_back(fovrt, t, env):
    t.set_shard(0, 2, 32)
    t.set_shard(0, 1)


def _trace_frame(fovrt, t, env):
    env.next_view(t)
    t.trace_frame(timing=False)


def _reconstruct_frame(fovrt, t, env):
    t.reconstruct_frame(timing=False)


def _geometry_launch(fovrt, t, env):
    t.geometry_launch()


def _rays_before(fovrt, t, env):
    env.rays = ray_batch(fovrt)
    env.ray_ref = t.trace_rays(env.rays, "closest")


def _trace_rays(fovrt, t, env):
    if env.rays is None:
        env.rays = ray_batch(fovrt)
    hits = t.trace_rays(env.rays, "closest")
    env.obs.append(("trace_rays", {"hits": hits.view(np.float32).reshape(-1, 4).copy(),
                                   "at_rest": np.array([env.geometry_at_rest], np.uint8)}))


OWN_WRITES = ("JFA_COORD", "JFA_COLOR", "WEIGHT", "MASK", "DEPTH")
PATTERN_WRITES = ("SHADING", "JFA_COLOR", "HISTORY_CACHE", "NORMAL", "DIFFUSE", "EXTRA")
VIEWS = ("JFA_COORD", "JFA_COLOR", "EXTRA", "HISTORY")

DISTURBERS = (
    [Step("nothing", _nothing), Step("snapshot_restore", _snapshot_restore), Step("restore_earlier", _restore_earlier)]
    + [Step(f"write_{n}_own_bytes", _write_own(n)) for n in OWN_WRITES]
    + [Step(f"write_{n}_pattern", _write_pattern(n)) for n in PATTERN_WRITES]
    + [Step(f"view_{n}", _view(n)) for n in VIEWS]
    + [Step("set_gaze", _set_gaze), Step("next_camera", _next_camera), Step("mask_mode_0", _mask_mode_0),
       Step("mask_mode_5_radius", _mask_mode_5), Step("mask_mode_6_caller_mask", _mask_mode_6),
       Step("move_model_refit", _move_model), Step("hide_model", _hide_model),
       Step("recon_chains_2_frame_3", _recon_chains), Step("shard_2_and_back", _shard_and_back),
       Step("trace_frame", _trace_frame), Step("reconstruct_frame", _reconstruct_frame),
       Step("geometry_launch", _geometry_launch), Step("trace_rays", _trace_rays, before_prefix=_rays_before)])
RESTORES = ("snapshot_restore", "restore_earlier")

# The disturbers that touch history, masks or the camera: also run under the latency and timed prefixes.
HISTORY_MASK_CAMERA = (
    "nothing", "snapshot_restore", "restore_earlier", "write_HISTORY_CACHE_pattern", "write_MASK_own_bytes",
    "write_WEIGHT_own_bytes", "write_DEPTH_own_bytes", "view_HISTORY", "set_gaze", "next_camera", "mask_mode_0",
    "mask_mode_5_radius", "mask_mode_6_caller_mask", "recon_chains_2_frame_3", "trace_frame")


# ---------------------------------------------------------------------------------------------------------------
# Observers: something that reads through the flags, then raw reads of what it produced. jfa_from: the observer ran
# JumpFlooding over the SHADING it read under that name; sibson: it ran Sibson (the JFA outputs are read after it,
# for the oracle).
# ---------------------------------------------------------------------------------------------------------------
class Observer(Step):
    def __init__(self, name, fn, ran_jfa=False, ran_sibson=False):
        super().__init__(name, fn)
        self.ran_jfa, self.ran_sibson = ran_jfa, ran_sibson


def _read(name):
    def run(fovrt, t, env):
        observe(fovrt, t, env, f"read_{name}", [name])
    return run


def _sibson_alone(fovrt, t, env):
    fovrt.SibsonInterpolation(t).render()
    observe(fovrt, t, env, "sibson_alone", ["SIBSON", "JFA_COORD", "JFA_COLOR"])


def _jfa_sibson(fovrt, t, env):
    shading = raw_read(fovrt, t, "SHADING")
    fovrt.JumpFlooding(t).render(fovrt.TextureName.SHADING)
    fovrt.SibsonInterpolation(t).render()
    observe(fovrt, t, env, "jfa_sibson", ["SIBSON", "JFA_COORD", "JFA_COLOR"], {"SHADING": shading})


def _atrous_jfa_color(fovrt, t, env):
    TN = fovrt.TextureName
    fovrt.ATrous(t).render(1, TN.POSITION, TN.NORMAL, TN.JFA_COLOR)
    observe(fovrt, t, env, "atrous_of_JFA_COLOR", ["ATROUS"])


def _copy_jfa_coord(fovrt, t, env):
    import torch
    out = torch.empty(t.width * t.height * 4, dtype=torch.float32, device="cuda")
    t.copy_buffer(fovrt.TextureName.JFA_COORD, out.data_ptr(), out.numel() * 4)
    env.obs.append(("copy_JFA_COORD", {"JFA_COORD": out.cpu().numpy().reshape(t.height, t.width, 4)}))


def _stage_front(fovrt, t, env):
    t.sampling_launch()
    t.optimize_launch()
    t.shading_launch()
    observe(fovrt, t, env, "sampling_optimize_shading", ["SHADING", "HISTORY_CACHE", "MASK"])


FRAME_READS = ["SHADING", "HISTORY_CACHE", "DEPTH_CACHE", "MASK", "JFA_COLOR", "SIBSON", "PULLPUSH", "ATROUS", "JFA_COORD"]


def _frame(mode):
    def run(fovrt, t, env):
        t.set_pipeline_mode(mode)
        env.next_view(t)
        t.frame(timing=False)
        observe(fovrt, t, env, "frame_latency" if mode else "frame_throughput", FRAME_READS)
    return run


OBSERVERS = [
    Observer("read_EXTRA", _read("EXTRA")), Observer("read_JFA_COORD", _read("JFA_COORD")),
    Observer("read_JFA_COLOR", _read("JFA_COLOR")),
    Observer("sibson_alone", _sibson_alone, ran_sibson=True),
    Observer("jfa_sibson", _jfa_sibson, ran_jfa=True, ran_sibson=True),
    Observer("atrous_of_JFA_COLOR", _atrous_jfa_color), Observer("copy_JFA_COORD", _copy_jfa_coord),
    Observer("sampling_optimize_shading", _stage_front),
    Observer("frame_throughput", _frame(0), ran_jfa=True, ran_sibson=True),
    Observer("frame_latency", _frame(1), ran_jfa=True, ran_sibson=True),
]

BY_NAME = {s.name: s for s in PREFIXES + DISTURBERS + OBSERVERS}


# ---------------------------------------------------------------------------------------------------------------
# MATRIX: (prefix, disturber, observer) names. Every pair under the two main prefixes; under the latency and timed
# prefixes every pair of the disturbers in HISTORY_MASK_CAMERA.
# ---------------------------------------------------------------------------------------------------------------
def build_matrix():
    out = []
    for p in PREFIXES:
        for d in DISTURBERS:
            if p.name not in MAIN_PREFIXES and d.name not in HISTORY_MASK_CAMERA:
                continue
            out.extend((p.name, d.name, o.name) for o in OBSERVERS)
    return out


MATRIX = build_matrix()

# Cases the API refuses with FovrtError, by name: (prefix, disturber, observer) -> the code every arm must report.
# None today: every step sets up what its calls need (the caller mask before mode 6, visibility enabled before a
# model is hidden, no ray budget), so a refusal met on the device is a failure until it is listed here with its reason.
REFUSED = {}
MAX_REFUSED_FRACTION = 0.05


def matrix_groups():
    """The parametrisation of the GPU test: (prefix, disturber) -> the observers looped inside one test."""
    groups = {}
    for p, d, o in MATRIX:
        groups.setdefault((p, d), []).append(o)
    return groups


# ---------------------------------------------------------------------------------------------------------------
# WALKS: seeded random walks over disturbers and observers, an observer at least every fourth step. A walk is its
# seed: walk(seed) is (prefix name, [step names], knob subset of the third context).
# ---------------------------------------------------------------------------------------------------------------
WALK_STEPS = 30


def walk(seed, steps=WALK_STEPS):
    rng = np.random.default_rng(seed)
    prefix = PREFIXES[int(rng.integers(len(PREFIXES)))].name
    bits = int(rng.integers(1, 2 ** len(KNOBS) - 1))  # neither the default context (0) nor the plain one (all)
    knobs = tuple(k for i, k in enumerate(KNOBS) if bits >> i & 1)
    pool = DISTURBERS + OBSERVERS
    names, since = [], 0
    for _ in range(steps):
        s = OBSERVERS[int(rng.integers(len(OBSERVERS)))] if since == 3 else pool[int(rng.integers(len(pool)))]
        since = 0 if isinstance(s, Observer) else since + 1
        names.append(s.name)
    return prefix, names, knobs


# Ordered pairs (a disturber immediately followed by an observer) the walks must meet at least once between them.
MUST_MEET = (
    [(r, o) for r in RESTORES for o in ("sibson_alone", "read_JFA_COORD")]
    + [("recon_chains_2_frame_3", o) for o in ("sibson_alone", "read_JFA_COORD", "frame_throughput")]
    + [(d, "sibson_alone") for d in ("view_JFA_COORD", "view_JFA_COLOR", "write_JFA_COORD_own_bytes",
                                     "write_JFA_COLOR_own_bytes", "write_JFA_COLOR_pattern")]
    + [("write_JFA_COLOR_pattern", "read_JFA_COORD"), ("view_EXTRA", "read_EXTRA"), ("write_EXTRA_pattern", "read_EXTRA")])


def pairs_met(seeds, steps=WALK_STEPS):
    met = set()
    for s in seeds:
        names = walk(s, steps)[1]
        met.update(zip(names, names[1:]))
    return met


def choose_seeds(n=16, candidates=range(4000), steps=WALK_STEPS):
    """n seeds whose walks meet every pair of MUST_MEET: greedily the seed that meets most of what is still missing
    (ties: the smallest), then the smallest unused seeds. How WALK_SEEDS below was made; None when n walks of this
    length cannot do it."""
    missing, seeds = set(MUST_MEET), []
    per = {s: pairs_met([s], steps) & set(MUST_MEET) for s in candidates}
    while missing and len(seeds) < n:
        best = max(per, key=lambda s: (len(per[s] & missing), -s))
        if not per[best] & missing:
            return None
        seeds.append(best)
        missing -= per.pop(best)
    if missing:
        return None
    seeds += [s for s in candidates if s not in seeds][:n - len(seeds)]
    return sorted(seeds)


WALK_SEEDS = (0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 374, 387, 580, 1667, 2088)  # choose_seeds(), written out
WALKS = [(s,) + walk(s) for s in WALK_SEEDS]
