"""Cases for the trace half's tests away from the preset cameras (pure numpy, no GPU): views with the
primary-hit class mix each one must deliver, screen sizes, tiny and thin shapes, parameter sets, and the helpers
the CPU and GPU tests share (camera, camera_rays_np, classes_np, and a restatement of the device's slab test).

Shapes are (W, H); images are (H, W, 4) float32, row 0 first. The views' class shares were measured with the
oracle at 64x48, detail 1; tests/test_cpu_trace_cases.py asserts them as conditions of the cases."""
import numpy as np

import ptx_np

F = np.float32

# name -> (scene, eye, target, up). Classes: 0 refraction, 1 reflection, 2 diffuse, 3 miss.
_UP = (0.0, 1.0, 0.0)
VIEWS = {
    # box scene (14 triangles: diffuse ground, glass box around (-3.5, 0.7, 1.2))
    "sky": (0, (0.0, 1.0, 5.0), (0.0, 30.0, 5.001), _UP),            # every pixel a miss: classes 0-2 empty
    "box_close": (0, (-3.5, 0.7, 2.3), (-3.5, 0.7, 1.2), _UP),       # every pixel refraction: classes 1-3 empty
    "inside_box": (0, (-3.5, 0.7, 1.2), (-1.5, 0.9, 1.0), _UP),      # eye inside the glass: first hit a back face
    # straight down along -y with up = -z, eye and target on binary fractions off the axes: column W/2 has
    # d.x = 0, row H/2 has d.z = 0, the centre both; the ground's boxes straddle 0 and the eye on x and on z
    "down_axis": (0, (0.5, 6.0, 0.25), (0.5, 0.0, 0.25), (0.0, 0.0, -1.0)),
    "grazing": (0, (0.0, -0.045, 9.0), (0.0, -0.05, -9.0), _UP),     # eye 5 mm above the ground
    "below": (0, (0.0, -3.0, 4.0), (0.0, 0.0, 0.0), _UP),            # the ground's back face everywhere
    # half a unit above the ground, looking along -z upside down: the left half of column W/2 has d.x = -0
    "upside_down": (0, (0.0, 0.5, 0.0), (0.0, 0.5, -4.0), (0.0, -1.0, 0.0)),
    # bunny scene (detail 1: 9,106 triangles; reflective earth, glass bunny and box, diffuse ground)
    "earth_close": (1, (0.0, 1.0, 1.1), (0.0, 1.0, 0.0), _UP),
    "along_z": (1, (0.0, 1.0, 6.0), (0.0, 1.0, 0.0), _UP),           # column W/2: d.x = 0; row H/2: d.y = 0
    "bunny_close": (1, (-1.5, 0.25, 1.75), (-1.5, 0.2, 1.2), _UP),
    "inside_bunny": (1, (-1.5, 0.2, 1.2), (0.0, 1.0, 0.0), _UP),
    # vokselia: the eye of test_reconstruction_chain_on_traced_frames (2.5 units up, along the ground)
    "street": (2, None, None, _UP),
}
VIEW_NAMES = list(VIEWS)
SCENE0_VIEWS = [n for n in VIEW_NAMES if VIEWS[n][0] == 0]

# The share of each class a view must deliver at 64x48 (oracle G-buffer): name -> {class: (lo, hi)}.
CONDITIONS = {
    "sky": {0: (0, 0), 1: (0, 0), 2: (0, 0), 3: (1, 1)},
    "box_close": {0: (1, 1), 1: (0, 0), 2: (0, 0), 3: (0, 0)},
    "inside_box": {0: (1, 1), 1: (0, 0), 2: (0, 0), 3: (0, 0)},
    "down_axis": {2: (0.9, 1)},
    "grazing": {2: (0.3, 1), 3: (0.3, 1)},
    "below": {2: (1, 1)},
    "upside_down": {2: (0.3, 1), 3: (0.3, 1)},
    "earth_close": {1: (0.7, 1)},
    "along_z": {0: (1e-9, 1), 1: (1e-9, 1), 2: (1e-9, 1), 3: (1e-9, 1)},
    "bunny_close": {0: (0.25, 1)},
    "inside_bunny": {0: (0.3, 1), 3: (0.1, 1)},
    "street": {2: (0.1, 1), 3: (0.1, 1)},
}

VIEW_SIZE = (64, 48)
RAGGED_SIZE = (100, 70)          # partial 8x8 tiles, 16x16 blocks and 16-pixel groups
RAGGED_VIEWS = ["along_z", "box_close"]
# views whose camera rays have a component of +-0 at 64x48 (test_cpu_trace_cases asserts it of each): the eye and
# the target share a coordinate, so column W/2 or row H/2 runs in a coordinate plane
ZERO_VIEWS = ["sky", "box_close", "down_axis", "grazing", "below", "upside_down", "earth_close", "along_z",
              "bunny_close"]
# every view at 64x48, two of them at 100x70 as well
VIEW_CASES = [(n,) + VIEW_SIZE for n in VIEW_NAMES] + [(n,) + RAGGED_SIZE for n in RAGGED_VIEWS]

# Narrower than a block, one pixel, one row, one column, one past a wave.
TINY_SHAPES = [(1, 1), (1, 40), (40, 1), (3, 2), (7, 5), (17, 5), (15, 17), (65, 3)]
MASK_MODES = [0, 1, 2, 3, 4]

# Parameter sets off the defaults (refraction_max_depth 16, diffuse_max_depth 1, light_power 810).
REFRACTION_DEPTHS = [2, 24, 25, 100]   # 24 / 25: either side of the device's item stack; 100: the reference's own
REFRACTION_VIEWS = ["inside_box", "bunny_close"]
DIFFUSE_DEPTHS = [2, 5]
DIFFUSE_DEPTH_SEQUENCE = [1, 4, 2]     # set_diffuse_max_depth between frames
LIGHT_POWERS = [100.0, 0.0]
PAN_VIEWS = ["along_z", "street"]
PAN_STEP = (0.01, 0.005, 0.0)          # the target's move per frame, as the pipelining tests pan

# The project's bars for entry 3 against the oracle (README, "Correctness contract").
SHADE_RMSE = 1e-3
SHADE_MAX = 5e-2
# The two sample-sum forms against each other (test_megakernel_tail_handoff's bars).
FORMS_RMSE = 1e-6
FORMS_MAX = 1e-4


def view_pose(fovrt, case):
    """(scene, eye, target, up) of a case; `street` takes the vokselia preset's eye, 2.5 units up."""
    scene, eye, target, up = VIEWS[case]
    if eye is None:
        pre = fovrt.Camera.preset(scene, 4, 4)
        eye = (float(pre.pos[0]), 2.5, float(pre.pos[2]))
        target = tuple(np.asarray(eye, np.float32) + np.array([1.0, -0.15, 0.3], np.float32))
    return scene, eye, target, up


def camera(fovrt, case, W, H):
    """A Camera on the case's view with the preset's projection (45 degrees, 0.1, 500.1)."""
    _scene, eye, target, up = view_pose(fovrt, case)
    cam = fovrt.Camera()
    cam.setRotation((1, 0, 0, 0))
    cam.setPosition(eye)
    cam.lookAt(target, up)
    cam.setProjectMode(fovrt.Camera.PM_Perspective, 45, 0.1, 500.1)
    cam.setScreen((W, H))
    cam.setViewport((0, 0, W, H))
    return cam


def camera_rays_np(uni, W, H):
    """Entry 0's camera rays (g_buffer_trace_camera.cu:95-100) in fp32 as its PTX forms them: ndc =
    fma(x / W, 2, -1), each row of inv_vp * (ndc, -1, 1) as fma(m3, 1, fma(m2, -1, fma(m0, x, m1 * y))),
    near = rcp(w) * row, d = normalize(near - eye) = v * rcp(sqrt(fma(z, z, fma(x, x, y * y))))
    (g_buffer_trace_camera.ptx:507-566). Returns (eye (3,), d (H, W, 3))."""
    fma = ptx_np.fma
    m = np.asarray(uni.inv_vp[:], F)
    eye = np.asarray(uni.eye[:], F)
    x = np.arange(W, dtype=F)[None, :].repeat(H, 0)
    y = np.arange(H, dtype=F)[:, None].repeat(W, 1)
    ndx = fma((x / F(W)).astype(F), F(2), F(-1))
    ndy = fma((y / F(H)).astype(F), F(2), F(-1))
    rows = [fma(m[4 * r + 3], F(1), fma(m[4 * r + 2], F(-1), fma(m[4 * r], ndx, (m[4 * r + 1] * ndy).astype(F))))
            for r in range(4)]
    with np.errstate(all="ignore"):
        inv = (F(1) / rows[3]).astype(F)
        v = [((rows[k] * inv).astype(F) - eye[k]).astype(F) for k in range(3)]
        n = (F(1) / np.sqrt(fma(v[2], v[2], fma(v[0], v[0], (v[1] * v[1]).astype(F))), dtype=F)).astype(F)
        d = np.stack([(c * n).astype(F) for c in v], -1)
    return eye, d


def closest_rays(eye, d, tmin=1e-3):
    """camera_rays_np's rays as rows (o, d, tmin, tmax) for OracleScene.closest."""
    n = d.shape[0] * d.shape[1]
    rays = np.empty((n, 8), F)
    rays[:, 0:3] = eye
    rays[:, 3:6] = d.reshape(-1, 3)
    rays[:, 6] = tmin
    rays[:, 7] = np.inf
    return rays


def classes_np(scene_arrays, prim):
    """The primary-hit class of each hit triangle index (any shape; < 0: a miss): the material type of the
    triangle's material, refraction -> 0, reflection -> 1, diffuse -> 2, miss -> 3."""
    prim = np.asarray(prim).astype(np.int64)
    flags = np.asarray(scene_arrays["flags"], np.int64)
    mats = np.asarray(scene_arrays["materials"], np.int64).reshape(-1, 2)
    mtype = mats[flags[np.clip(prim, 0, len(flags) - 1)] & 0xFF, 0]
    cls = np.array([2, 1, 0], np.uint8)[mtype]  # MAT_DIFFUSE 0, MAT_REFLECTION 1, MAT_REFRACTION 2
    return np.where(prim < 0, np.uint8(3), cls).astype(np.uint8)


def primary_classes(oracle_scene, scene_arrays, uni, W, H):
    """(classes (H, W) u8, hits (H, W, 4): t, prim, beta, gamma) of the oracle's closest hit on every camera ray."""
    eye, d = camera_rays_np(uni, W, H)
    hits = oracle_scene.closest(closest_rays(eye, d)).reshape(H, W, 4)
    return classes_np(scene_arrays, hits[..., 1]), hits


# The device's box tests on a ray (csrc/k_trace.hip: slab4_keys and root_hit), restated to show what the
# finite stand-in for 1 / +-0 is for. A plane distance is fma(plane, inv, -o * inv). With inv = +-inf the
# planes of a box that straddles both 0 and the origin on that axis come out as one NaN and one -inf.
def reciprocal_np(d, safe=True):
    """1 / d; with safe, +-2^100 where the reciprocal overflows (safe_rcp)."""
    with np.errstate(all="ignore"):
        r = (F(1) / np.asarray(d, F)).astype(F)
    return np.where(np.isinf(r), np.copysign(F(2.0 ** 100), r), r).astype(F) if safe else r


def box_reached_np(lo, hi, o, inv, tmin, tmax):
    """root_hit's form: per axis min / max of the two plane distances (fminf / fmaxf drop a NaN operand), the
    entry distance max over axes and tmin, the exit distance min over axes and tmax. lo, hi: (..., 3)."""
    lo, hi, o, inv = (np.asarray(a, F) for a in (lo, hi, o, inv))
    with np.errstate(all="ignore"):
        oi = (-o * inv).astype(F)
        p0, p1 = ptx_np.fma(lo, inv, oi), ptx_np.fma(hi, inv, oi)
        near = np.fmax(np.fmax.reduce(np.fmin(p0, p1), axis=-1), F(tmin))
        far = np.fmin(np.fmin.reduce(np.fmax(p0, p1), axis=-1), F(tmax))
    return near <= far
