"""The case set the CPU and GPU suites of the reprojected present share: screens, synthetic POSITION images and display
poses. Sources are the present suite's value set (present_warp_np.source)."""
import numpy as np

import present_warp_np as pwn

F = np.float32
# W, H, ow, oh: one texel; fewer texels than a lane row; one full wave row of lanes with 16-byte rows; more than one
# block of rows; wider than one block row of lanes, with a tail; a smaller output (four texels to a place)
SCREENS = [(1, 1, 1, 1), (7, 5, 7, 5), (64, 4, 64, 4), (100, 70, 100, 70), (259, 3, 259, 3), (100, 70, 50, 35)]
DEPTH, NEAR = 7.0, 4.0  # the plane's distance from the rendered camera, and the nearer plane's of case (b)
POSITIONS = ("a plane with misses", "b two planes", "c ties", "d all misses", "e non-finite and behind")
TIE_ROWS = 2  # case (c): every other row, texel 2 k + 1 has texel 2 k's position


def camera(fovrt, W, H):
    return pwn.case_camera(fovrt, W, H)


def axes(cam):
    """right, up, forward of the camera in world space, float64, from its view matrix."""
    V = cam._matrices()[0].astype(np.float64)
    return V[0, :3], V[1, :3], -V[2, :3]


def plane(cam, W, H, depth):
    """(H, W, 3) float32: the world points at view depth `depth` under the texel centres, unprojected in f64 and
    rounded once."""
    V, P = (m.astype(np.float64) for m in cam._matrices())
    x, y = np.meshgrid((np.arange(W) + 0.5) * 2 / W - 1, (np.arange(H) + 0.5) * 2 / H - 1)
    view = np.stack([x * depth / P[0, 0], y * depth / P[1, 1], np.full(x.shape, -depth), np.ones(x.shape)], -1)
    world = view @ np.linalg.inv(V).T
    return world[..., :3].astype(F)


def miss_block(W, H):
    """A block of texels at least two thick each way where the image has neighbours that way (a run of misses one
    texel thick between hits is a crack by the rule, not a hole); none on a screen narrower than four texels."""
    if W < 4:
        return slice(0, 0), slice(0, 0)
    return slice(H // 4, min(H, H // 4 + max(2, H // 4))), slice(W // 4, W // 4 + max(2, W // 4))


def position(fovrt, name, W, H):
    """The (H, W, 4) float32 POSITION image of a case; w = 1 as the G-buffer writes it."""
    cam = camera(fovrt, W, H)
    P = np.ones((H, W, 4), F)
    P[..., :3] = plane(cam, W, H, DEPTH)
    if name[0] in "ace":
        P[miss_block(W, H)] = (0, 0, 0, 1)  # exact misses
    if name[0] == "b":
        P[:, W // 3:max(2 * W // 3, W // 3 + 1), :3] = plane(cam, W, H, NEAR)[:, W // 3:max(2 * W // 3, W // 3 + 1)]
    if name[0] == "c":
        n = (W // 2) * 2
        P[::TIE_ROWS, 1:n:2] = P[::TIE_ROWS, 0:n:2]
    if name[0] == "d":
        P[...] = (0, 0, 0, 1)
    if name[0] == "e":
        _r, _u, fwd = axes(cam)
        flat = P.reshape(-1, 4)
        n = flat.shape[0]
        behind = (cam.pos.astype(np.float64) - 3.0 * fwd).astype(F)
        for k, bad in enumerate((np.nan, np.inf, -np.inf)):
            for ch in range(3):
                flat[(3 * k + ch) * 2 % n::23, ch] = bad  # one component of each kind, spread over the image
        flat[5 % n::17, :3] = behind
        flat[11 % n::29, :3] = cam.pos  # the eye itself: cw = 0
    return P


def displays(fovrt, cam):
    """[(name, display camera)]: the poses a frame is shown for."""
    right, _up, fwd = axes(cam)
    t = lambda axis, deg, move: pwn.turned(fovrt, cam, axis, deg, move)
    return [("equal", t(0, 0.0, (0, 0, 0))),
            ("closer 0.3", t(0, 0.0, 0.3 * fwd)),
            ("closer 1.0", t(0, 0.0, 1.0 * fwd)),
            ("farther", t(0, 0.0, -1.5 * fwd)),
            ("lateral", t(0, 0.0, 0.5 * right)),
            ("turn 2", t(1, 2.0, (0, 0, 0))),
            ("turn and shift", t(1, 2.0, 0.3 * right + 0.2 * fwd))]


def reprojections(fovrt, W, H, ow, oh):
    """[(name, PresentReproject)] of the display poses for one screen; the fallback is at the far plane."""
    cam = camera(fovrt, W, H)
    return [(name, fovrt.PresentReproject.from_poses(cam, d, W, H, ow, oh, 1.0)) for name, d in displays(fovrt, cam)]


def sources(W, H):
    """Four sources, one per presentable buffer."""
    return [pwn.source(W, H, k) for k in range(4)]
