"""A second restatement of the trace stages, written from the reference's device programs (not from
oracle/oracle.cpp): entry 0 (g_buffer_trace + the ray-type-0 closest hit g_diffuse + g_miss), entry 3
(ray_trace), the three ray-type-1 material programs with their shadow any-hits, and envmap_miss.

Test infrastructure only (the CPU suite checks oracle.gbuffer / oracle.shading against it). Scalar
fp32 arithmetic in numpy (every operation rounded to float32), with fma.rn wherever the reference's PTX
contracts (tests/ptx_np.py's transcription of each site supplies the arithmetic and CUDA's sinf / cosf /
atan2f / acosf), brute-force intersection against every triangle (the box preset has 14), the
reference's recursion as Python recursion.

Files followed (FR/ = /root/reference/Foveated Rendering using Ray Tracing/):
  FR/cuda/g_buffer_trace_camera.cu:84-151, FR/cuda/g_diffuse.cu:67-144, FR/cuda/gradientbg.cu:45-66,
  FR/cuda/fov_path_trace_camera.cu:72-176, FR/cuda/diffuse.cu:65-148,226-241, FR/cuda/reflection.cu:71-169,
  239-253, FR/cuda/refraction.cu:59-153, FR/cuda/triangle_mesh.cu:57-105,
  FR/cuda/device_include/intersection_refinement.h:37-99, shared_helper_funcs.h:179-188,341-373,
  shared_helper_math.h:8-21, random.h:31-67; material parameters FR/PathTracer.cpp:676-772, light :564-579.
OptiX 5.1 header intrinsics (not under /root/reference; their public form, SURVEY Appendix B.3/B.4, in
the form the compiled PTX gives them): intersect_triangle, normalize (v * (1 / sqrt(v.v))), faceforward,
reflect, refract, Onb, cosine_sample_hemisphere, fresnel_schlick, luminance, float3 / float
(multiplication by 1 / s), Matrix4x4 * float4.
Choices the reference leaves open, pinned the way the build's contract states them (SURVEY
Appendix A): textures bilinear with 8-bit fractions and REPEAT wrap (the CUDA texture unit's documented
filtering), uninitialised child payload fields (seed = the parent's, reflectance 0, done 0, importance 1),
an entry-0 miss writes position 0, the refraction recursion capped at refraction_max_depth, closest-hit
ties to the lowest triangle index, and the refractive shadow attenuation multiplied in f64 (independent of
the traversal order)."""
import ctypes
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ptx_np  # noqa: E402

f = np.float32

# powf ends in ex2.approx / rcp.approx in the PTX (unspecified bits): the platform libm's fp32 powf, as the
# build's contract defines it for the continuous shading stages. sinf / cosf / acosf /
# atan2f are CUDA's fma polynomials, transcribed in ptx_np.
_libm = ctypes.CDLL("libm.so.6")
_libm.powf.restype = ctypes.c_float
_libm.powf.argtypes = [ctypes.c_float] * 2


def sinf(x):
    return f(ptx_np.sinf(f(x)))


def cosf(x):
    return f(ptx_np.cosf(f(x)))


def acosf(x):
    return f(ptx_np.acosf(f(x)))


def powf(x, y):
    return f(_libm.powf(float(x), float(y)))


def atan2f(y, x):
    return f(ptx_np.atan2f(f(y), f(x)))


def fma(a, b, c):
    """fma.rn.f32 (one rounding)."""
    return f(ptx_np.fma(f(a), f(b), f(c)))


PI = f(3.14159265358979323846)
ONE_PI = f(0.318309886183790671538)
EPS = f(1e-3)  # scene_epsilon (FR/PathTracer.cpp:474)
MAT_DIFFUSE, MAT_REFLECTION, MAT_REFRACTION = 0, 1, 2


# ---- float3 helpers (tuples of np.float32; every operation rounds to fp32) ----
def v3(x, y, z):
    return (f(x), f(y), f(z))


def add(a, b):
    return (f(a[0] + b[0]), f(a[1] + b[1]), f(a[2] + b[2]))


def sub(a, b):
    return (f(a[0] - b[0]), f(a[1] - b[1]), f(a[2] - b[2]))


def mul(a, b):
    return (f(a[0] * b[0]), f(a[1] * b[1]), f(a[2] * b[2]))


def scale(a, s):
    s = f(s)
    return (f(a[0] * s), f(a[1] * s), f(a[2] * s))


def neg(a):
    return (-a[0], -a[1], -a[2])


def dot(a, b):
    """optix::dot as nvcc contracts it: fma(z, z', fma(x, x', y * y')) (triangle_mesh.ptx:384-388)."""
    return fma(a[2], b[2], fma(a[0], b[0], f(a[1] * b[1])))


def fma3(s, b, c):
    """fma(s, b, c) per component (s a scalar or a tuple)."""
    s = s if isinstance(s, tuple) else (s, s, s)
    return (fma(s[0], b[0], c[0]), fma(s[1], b[1], c[1]), fma(s[2], b[2], c[2]))


def cross(a, b):
    return (f(f(a[1] * b[2]) - f(a[2] * b[1])), f(f(a[2] * b[0]) - f(a[0] * b[2])), f(f(a[0] * b[1]) - f(a[1] * b[0])))


def length(v):
    return np.sqrt(dot(v, v), dtype=np.float32)


def normalize(v):
    return scale(v, f(f(1) / length(v)))


def fmax3(v):
    return max(v[0], v[1], v[2])


def faceforward_neg(n, d, nref):
    """faceforward(n, -d, nref): the sign of ((-(nref.y d.y)) - d.x nref.x) - nref.z d.z, unfused
    (g_diffuse.ptx:199-210)."""
    s = f(f(f(-f(nref[1] * d[1])) - f(d[0] * nref[0])) - f(nref[2] * d[2]))
    return scale(n, np.copysign(f(1), s))


def reflect(i, n):
    """i - (n + n) dot(n, i) (refraction.ptx:498-508)."""
    return sub(i, scale(add(n, n), dot(n, i)))


def refract(i, n, ior):
    """optix::refract: (ok, t)."""
    nn, c = n, dot(i, n)
    if c > 0:
        eta, nn, c = f(ior), neg(n), -c
    else:
        eta = f(f(1) / f(ior))
    k = f(f(1) - f(f(eta * eta) * f(f(1) - f(c * c))))
    if k < 0:
        return False, v3(0, 0, 0)
    return True, normalize(sub(scale(i, eta), scale(nn, fma(c, eta, np.sqrt(k, dtype=np.float32)))))


def fresnel_schlick(c, e, lo, hi):
    """max(lo, min(fma(hi - lo, pow, lo), hi)) (refraction.ptx:611-614)."""
    p = powf(max(f(0), f(f(1) - c)), e)
    return max(f(lo), min(fma(f(f(hi) - f(lo)), p, f(lo)), f(hi)))


def luminance(c):
    return dot(c, v3(0.30, 0.59, 0.11))


def cosine_sample_hemisphere(u1, u2):
    r = np.sqrt(u1, dtype=np.float32)
    phi = f(f(f(2) * PI) * u2)
    x = f(r * cosf(phi))
    y = f(r * sinf(phi))
    return (x, y, np.sqrt(max(f(0), f(f(f(1) - f(x * x)) - f(y * y))), dtype=np.float32))


def onb_inverse_transform(n, p):
    if abs(n[0]) > abs(n[2]):
        b = (-n[1], n[0], f(0))
    else:
        b = (f(0), -n[2], n[1])
    b = normalize(b)
    t = cross(b, n)
    return fma3(p[2], n, fma3(p[1], b, scale(t, p[0])))  # diffuse.ptx:556-580


def tea16(v0, v1):
    M = 0xFFFFFFFF
    s0 = 0
    for _ in range(16):
        s0 = (s0 + 0x9e3779b9) & M
        v0 = (v0 + (((((v1 << 4) & M) + 0xa341316c) & M) ^ ((v1 + s0) & M) ^ (((v1 >> 5) + 0xc8013ea4) & M))) & M
        v1 = (v1 + (((((v0 << 4) & M) + 0xad90777d) & M) ^ ((v0 + s0) & M) ^ (((v0 >> 5) + 0x7e95761e) & M))) & M
    return v0


class Rng:
    """lcg / rnd (random.h:49-63) on a mutable seed."""

    def __init__(self, seed):
        self.seed = seed & 0xFFFFFFFF

    def rnd(self):
        self.seed = (1664525 * self.seed + 1013904223) & 0xFFFFFFFF
        return f(f(self.seed & 0xFFFFFF) / f(16777216.0))


def mat_vec(m, v):
    """optix::Matrix4x4 * float4, row-major m (16 floats), each row fma(m3, w, fma(m2, z, fma(m0, x, m1 * y)))
    (g_diffuse.ptx:659-685)."""
    m = [f(x) for x in m]
    return tuple(fma(m[4 * r + 3], v[3], fma(m[4 * r + 2], v[2], fma(m[4 * r], v[0], f(m[4 * r + 1] * v[1]))))
                 for r in range(4))


def div_w(tmp):
    """float3 / float: multiplication by rcp(w) (g_buffer_trace_camera.ptx:545-548)."""
    inv = f(f(1) / tmp[3])
    return (f(tmp[0] * inv), f(tmp[1] * inv), f(tmp[2] * inv))


def _bits(x):
    return int(np.asarray(x, np.float32).view(np.int32))


def _from_bits(i):
    return np.asarray(np.int32(((i + 2 ** 31) % 2 ** 32) - 2 ** 31)).view(np.float32)[()]


def _trunc_int(x):
    """int(float): truncation toward zero (the values here stay far inside the int range)."""
    return int(np.trunc(np.float64(x)))


def _offset(h, n):
    """intersection_refinement.h:47-72: 8192 ulps along the normal, or 1e-4 near zero."""
    eps, off = f(1.0e-4), f(4096.0 * 2.0)
    out = []
    for k in range(3):
        if (_bits(h[k]) & 0x7FFFFFFF) < _bits(eps):
            out.append(fma(n[k], eps, h[k]))
        else:
            out.append(_from_bits(_bits(h[k]) + _trunc_int(f(np.copysign(off, h[k]) * n[k]))))
    return tuple(out)


def refine_and_offset_hitpoint(original, direction, normal, p):
    """intersection_refinement.h:80-99: (back, front); refined = fma(refined_t, d, original)."""
    refined_t = f(-dot(normal, sub(original, p)) / dot(normal, direction))
    refined = fma3(refined_t, direction, original)
    if dot(direction, normal) > 0:
        return _offset(refined, normal), _offset(refined, neg(normal))
    return _offset(refined, neg(normal)), _offset(refined, normal)


class SceneNp:
    """A scene dict (fovrt.Scene(cfg).arrays()) as float32 arrays; textures bilinear with 8-bit fractions
    and REPEAT wrap (sutil::loadTexture's sampler, FR/PathTracer.cpp:857-870's house convention)."""

    def __init__(self, a, refraction_max_depth=16, diffuse_max_depth=1):
        self.pos = np.asarray(a["pos"], np.float32).reshape(-1, 3, 3)
        self.nrm = np.asarray(a["nrm"], np.float32).reshape(-1, 3, 3)
        self.uv = np.asarray(a["uv"], np.float32).reshape(-1, 3, 2)
        self.flags = np.asarray(a["flags"], np.int64)
        self.mats = np.asarray(a["materials"], np.int64).reshape(-1, 2)
        self.tex = [np.asarray(t, np.float32) for t in a["textures"]]
        self.envmap = int(a["envmap"])
        L = np.asarray(a["light"], np.float32)
        self.light_pos, self.light_v1, self.light_v2 = tuple(L[0:3]), tuple(L[3:6]), tuple(L[6:9])
        self.light_n, self.light_e = tuple(L[9:12]), tuple(L[12:15])
        self.refraction_max_depth = refraction_max_depth
        self.diffuse_max_depth = diffuse_max_depth
        P = self.pos
        self.p0, self.p1, self.p2 = P[:, 0], P[:, 1], P[:, 2]
        self.e0 = (self.p1 - self.p0).astype(np.float32)
        self.e1 = (self.p0 - self.p2).astype(np.float32)
        self.n = np.stack([self.e1[:, 1] * self.e0[:, 2] - self.e1[:, 2] * self.e0[:, 1],
                           self.e1[:, 2] * self.e0[:, 0] - self.e1[:, 0] * self.e0[:, 2],
                           self.e1[:, 0] * self.e0[:, 1] - self.e1[:, 1] * self.e0[:, 0]], 1).astype(np.float32)

    def material(self, k):
        m = int(self.flags[k]) & 0xFF
        return int(self.mats[m, 0]), int(self.mats[m, 1])

    def tex2d(self, ti, u, v):
        img = self.tex[ti]
        h, w = img.shape[:2]
        tx, ty = f(f(u * f(w)) - f(0.5)), f(f(v * f(h)) - f(0.5))
        x0, y0 = np.floor(tx), np.floor(ty)
        a, b = f(tx - x0), f(ty - y0)
        a = f(np.floor(f(f(a * f(256)) + f(0.5))) * f(1.0 / 256))
        b = f(np.floor(f(f(b * f(256)) + f(0.5))) * f(1.0 / 256))
        ix, iy = int(np.clip(x0, -2 ** 31, 2 ** 31 - 1)), int(np.clip(y0, -2 ** 31, 2 ** 31 - 1))
        X0, X1, Y0, Y1 = ix % w, (ix + 1) % w, iy % h, (iy + 1) % h
        one = f(1)
        # the CUDA programming guide's linear filter: (1-a)(1-b) T[i,j] + a(1-b) T[i+1,j] + (1-a)b T[i,j+1] + ab T[i+1,j+1]
        ws = [f(f(one - a) * f(one - b)), f(a * f(one - b)), f(f(one - a) * b), f(a * b)]
        ts = [img[Y0, X0], img[Y0, X1], img[Y1, X0], img[Y1, X1]]
        acc = (ts[0] * ws[0]).astype(np.float32)
        for t, wgt in zip(ts[1:], ws[1:]):
            acc = (acc + (t * wgt).astype(np.float32)).astype(np.float32)
        return acc

    # ---- triangle_mesh.cu: intersect_triangle over every triangle ----
    def _tests(self, o, d, tmin, tmax):
        o, d = np.asarray(o, np.float32), np.asarray(d, np.float32)
        with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
            # the contracted dots of triangle_mesh.ptx:383-416
            F = ptx_np.fma
            n = self.n
            den = F(n[:, 2], d[2], F(n[:, 0], d[0], (n[:, 1] * d[1]).astype(np.float32)))
            r = (f(1) / den).astype(np.float32)
            q = (self.p0 - o).astype(np.float32)
            e2 = (r[:, None] * q).astype(np.float32)
            i = np.stack([d[1] * e2[:, 2] - d[2] * e2[:, 1], d[2] * e2[:, 0] - d[0] * e2[:, 2],
                          d[0] * e2[:, 1] - d[1] * e2[:, 0]], 1).astype(np.float32)
            e0, e1 = self.e0, self.e1
            beta = F(e1[:, 2], i[:, 2], F(e1[:, 0], i[:, 0], (e1[:, 1] * i[:, 1]).astype(np.float32)))
            gamma = F(e0[:, 2], i[:, 2], F(e0[:, 0], i[:, 0], (e0[:, 1] * i[:, 1]).astype(np.float32)))
            t = F(n[:, 2], e2[:, 2], F(n[:, 0], e2[:, 0], (n[:, 1] * e2[:, 1]).astype(np.float32)))
            hit = (t < f(tmax)) & (t > f(tmin)) & (beta >= 0) & (gamma >= 0) & ((beta + gamma).astype(np.float32) <= 1)
        return hit, t, beta, gamma

    def closest(self, o, d, tmin, tmax=np.inf):
        hit, t, beta, gamma = self._tests(o, d, tmin, tmax)
        if not hit.any():
            return None
        tt = np.where(hit, t, np.float32(np.inf))
        k = int(np.argmin(tt))  # the first of equal distances: the lowest triangle index
        return k, f(t[k]), f(beta[k]), f(gamma[k])

    def attributes(self, k, t, beta, gamma, o, d):
        """mesh_intersect_refine's attributes of hit k."""
        geo = normalize(tuple(self.n[k]))
        w = f(f(f(1) - beta) - gamma)
        fl = int(self.flags[k])
        if fl & 0x100:  # fma(w, n0, fma(b, n1, g n2)) (triangle_mesh.ptx:478-488)
            n0, n1, n2 = (tuple(x) for x in self.nrm[k])
            shading = normalize(fma3(w, n0, fma3(beta, n1, scale(n2, gamma))))
        else:
            shading = geo
        if fl & 0x200:
            t0, t1, t2 = self.uv[k]
            uv = tuple(fma(w, t0[c], fma(beta, t1[c], f(gamma * t2[c]))) for c in range(2))
        else:
            uv = (f(0), f(0))
        hitp = fma3(t, d, o)  # triangle_mesh.ptx:559-564
        back, front = refine_and_offset_hitpoint(hitp, d, geo, tuple(self.p0[k]))
        return dict(geo=geo, shading=shading, uv=uv, front=front, back=back, t=t)

    def shadow(self, o, d, tmin, tmax):
        """Ray type 2 with the any-hit programs of every triangle it crosses (diffuse.cu:226-241,
        reflection.cu:239-253, refraction.cu:144-153)."""
        hit, t, beta, gamma = self._tests(o, d, tmin, tmax)
        att = 1.0
        for k in np.nonzero(hit)[0]:
            mtype, _ = self.material(int(k))
            if mtype != MAT_REFRACTION:
                return v3(0, 0, 0)
            a = self.attributes(int(k), f(t[k]), f(beta[k]), f(gamma[k]), o, d)
            nDi = abs(dot(normalize(a["shading"]), d))
            att *= float(f(f(1) - fresnel_schlick(nDi, 5.0, 0.0, 1.0)))
        return v3(att, att, att)

    def kd(self, k, uv):
        _, ti = self.material(k)
        return tuple(self.tex2d(ti, uv[0], uv[1])[:3])


def _light_sample(sc, z1, z2):
    """fma(z2, v2, fma(z1, v1, light_position)) (diffuse.ptx:672-679)."""
    return fma3(z2, sc.light_v2, fma3(z1, sc.light_v1, sc.light_pos))


def _light_weight(sc, nDl, LnDl, Ldist):
    A = length(cross(sc.light_v1, sc.light_v2))
    return f(f(f(nDl * LnDl) * A) / f(f(PI * Ldist) * Ldist))


# ---- ray type 1 (entry 3's radiance rays) ----
def trace_radiance(sc, o, d, prd):
    h = sc.closest(o, d, EPS)
    if h is None:
        envmap_miss(sc, d, prd)
        return
    k, t, beta, gamma = h
    a = sc.attributes(k, t, beta, gamma, o, d)
    mtype, _ = sc.material(k)
    if mtype == MAT_DIFFUSE:
        ch_diffuse(sc, k, a, o, d, prd)
    elif mtype == MAT_REFLECTION:
        ch_reflection(sc, k, a, o, d, prd)
    else:
        ch_refraction(sc, k, a, o, d, prd)


def child_prd(parent, depth, importance=1.0, reflectance=0.0, result=0.0):
    """A child payload: the fields its caller leaves uninitialised pinned as the build's contract states."""
    return dict(depth=depth, seed=parent["seed"], done=False, importance=f(importance),
                reflectance=v3(reflectance, reflectance, reflectance), result=v3(result, result, result))


def envmap_miss(sc, d, prd):
    """gradientbg.cu:57-66."""
    prd["done"] = True
    theta = atan2f(d[0], d[2])
    phi = f(f(PI * f(0.5)) - acosf(d[1]))
    u = f(f(theta + PI) * f(f(0.5) * ONE_PI))
    v = f(f(0.5) * f(f(1) + sinf(phi)))  # CUDA's atan2f / acosf / sinf (gradientbg.ptx:102-212)
    prd["result"] = scale(tuple(sc.tex2d(sc.envmap, u, v)[:3]), f(2))


def ch_diffuse(sc, k, a, o, d, prd):
    """diffuse.cu:65-148."""
    wsn, wgn = normalize(a["shading"]), normalize(a["geo"])
    ffn = faceforward_neg(wsn, d, wgn)
    rng = Rng(prd["seed"])
    z1, z2 = rng.rnd(), rng.rnd()
    prd["seed"] = rng.seed
    diff_dir = onb_inverse_transform(ffn, cosine_sample_hemisphere(z1, z2))
    hitp = a["front"]
    Kd = sc.kd(k, a["uv"])
    shadow_result = v3(0, 0, 0)
    lp = _light_sample(sc, z1, z2)
    Ldist, L = length(sub(lp, hitp)), normalize(sub(lp, hitp))
    nDl, LnDl = dot(ffn, L), dot(sc.light_n, L)
    if nDl > 0 and LnDl > 0:
        att = sc.shadow(hitp, L, EPS, Ldist)
        if fmax3(att) > 0:
            w = _light_weight(sc, nDl, LnDl, Ldist)
            shadow_result = fma3(att, scale(sc.light_e, w), shadow_result)  # diffuse.ptx:741-746
    prd["reflectance"] = mul(Kd, shadow_result)
    result = mul(Kd, shadow_result)
    depth = 0
    if prd["done"]:
        result = add(result, mul(Kd, shadow_result))
    if prd["depth"] < sc.diffuse_max_depth - 1:
        c = child_prd(prd, prd["depth"] + 1)
        trace_radiance(sc, hitp, diff_dir, c)
        result = add(result, c["reflectance"])
        depth = c["depth"]
    prd["depth"] = depth + 1
    prd["result"] = result


def ch_reflection(sc, k, a, o, d, prd):
    """reflection.cu:71-169 (Ks 1, phong_exp 88, reflectivity_n 0.05, importance_cutoff 1e-2,
    reflection_max_depth 4: FR/PathTracer.cpp:728-737)."""
    wsn, wgn = normalize(a["shading"]), normalize(a["geo"])
    ffn = faceforward_neg(wsn, d, wgn)
    hitp = a["front"]
    Kd = sc.kd(k, a["uv"])
    shadow_result = v3(0, 0, 0)
    rng = Rng(prd["seed"])
    z1, z2 = rng.rnd(), rng.rnd()
    prd["seed"] = rng.seed
    lp = _light_sample(sc, z1, z2)
    Ldist, L = length(sub(lp, hitp)), normalize(sub(lp, hitp))
    nDl, LnDl = dot(ffn, L), dot(sc.light_n, L)
    if nDl > 0 and LnDl > 0:
        att = sc.shadow(hitp, L, EPS, Ldist)
        if fmax3(att) > 0:
            w = _light_weight(sc, nDl, LnDl, Ldist)
            Lc = mul(att, scale(sc.light_e, w))
            shadow_result = fma3(scale(Kd, nDl), Lc, shadow_result)  # reflection.ptx:386-391
            H = normalize(sub(L, d))
            nDh = dot(ffn, H)
            if nDh > 0:
                p = powf(nDh, 88)
                shadow_result = fma3(mul(Lc, v3(1, 1, 1)), (p, p, p), shadow_result)
    prd["reflectance"] = mul(prd["reflectance"], mul(Kd, shadow_result))
    result = mul(Kd, shadow_result)
    c_ = f(-dot(ffn, d))
    r = tuple(fresnel_schlick(c_, 5.0, 0.05, 1.0) for _ in range(3))
    importance = f(prd["importance"] * luminance(r))
    if importance > f(1e-2) and prd["depth"] < 4:
        c = child_prd(prd, prd["depth"] + 1, importance=importance)
        trace_radiance(sc, hitp, reflect(d, ffn), c)
        result = fma3(r, c["reflectance"], result)  # reflection.ptx:833-835
    prd["result"] = result


def _refr_add(result, w, c):
    """result += w * c as refraction.ptx:660-746 forms it: x, y unfused, z as fma(c.z, w.z, result.z)."""
    return (f(result[0] + f(w[0] * c[0])), f(result[1] + f(w[1] * c[1])), fma(c[2], w[2], result[2]))


def ch_refraction(sc, k, a, o, d, prd):
    """refraction.cu:59-142 (IOR 1.4, fresnel 3 / 0.1 / 1, cutoff colour (0.34, 0.55, 0.85), importance_cutoff
    1e-2, extinction log(1) = 0: FR/PathTracer.cpp:748-762; refraction and reflection depth capped at
    refraction_max_depth)."""
    h = fma3(a["t"], d, o)  # refraction.ptx:279-281
    n = normalize(a["shading"])
    i = d
    Kd = sc.kd(k, a["uv"])
    cutoff = v3(0.34, 0.55, 0.85)
    one3 = v3(1, 1, 1)
    beer = one3  # exp(extinction_constant * t_hit) with extinction_constant = log(1) = 0: exactly 1
    reflection = f(1)
    result = v3(0, 0, 0)
    cap = sc.refraction_max_depth
    if prd["depth"] < cap:
        ok, t = refract(i, n, 1.4)
        if ok:
            cos_theta = dot(i, n)
            cos_theta = -cos_theta if cos_theta < 0 else dot(t, n)
            reflection = fresnel_schlick(cos_theta, 3.0, 0.1, 1.0)
            importance = f(f(prd["importance"] * f(f(1) - reflection)) * luminance(mul(one3, beer)))
            if importance > f(1e-2):
                c = child_prd(prd, prd["depth"] + 1, importance=importance)
                trace_radiance(sc, h, t, c)
                result = _refr_add(result, scale(one3, f(f(1) - reflection)), c["result"])
            else:
                result = _refr_add(result, scale(one3, f(f(1) - reflection)), cutoff)
    if prd["depth"] < cap:
        r = reflect(i, n)
        importance = f(f(prd["importance"] * reflection) * luminance(mul(one3, beer)))
        if importance > f(1e-2):
            c = child_prd(prd, prd["depth"] + 1, importance=importance)
            trace_radiance(sc, h, r, c)
            result = _refr_add(result, scale(one3, reflection), c["result"])
        else:
            result = _refr_add(result, scale(one3, reflection), cutoff)
    result = mul(result, beer)
    prd["result"] = mul(Kd, result)
    prd["done"] = True


def tonemap(c):
    """Uncharted2ToneMapping (shared_helper_funcs.h:354-373) as fov_path_trace_camera.ptx:602-630 forms it:
    x = c + c, U(x) = fma(x, fma(x, A, C B), D E) / fma(x, fma(x, A, B), D F) - E / F, times the folded
    1 / U(11.2), then powf(., 2.2)."""
    A, B, C, D, E, F = f(0.15), f(0.50), f(0.10), f(0.20), f(0.02), f(0.30)

    def U(x):
        return f(f(fma(x, fma(x, A, f(C * B)), f(D * E)) / fma(x, fma(x, A, B), f(D * F))) - f(E / F))
    white = ptx_np.hexf(0x3FB0852E)
    return tuple(powf(f(U(f(x + x)) * white), f(2.2)) for x in c)


def _color_to_accumulated(c):
    if c[3] > 0:
        return np.array([f(c[0] / c[3]), f(c[1] / c[3]), f(c[2] / c[3]), f(1)], np.float32)
    return np.array(c, np.float32)


def _round_u32(x):
    r = np.float64(np.trunc(np.float64(x) + np.copysign(0.5, np.float64(x))))  # roundf: half away from zero
    return int(min(max(r, 0.0), 4294967295.0)) if r == r else 0


def gbuffer_np(sc, cam, W, H, frame):
    """Entry 0 (g_buffer_trace_camera.cu:84-151, g_diffuse.cu:67-144, gradientbg.cu:45-51)."""
    out = {k: np.zeros((H, W, 4), np.float32) for k in ("position", "normal", "depth", "diffuse", "weight")}
    from trace_cases import camera_rays_np  # the camera ray's arithmetic, shared with the off-preset cases
    prev_vp = list(cam.prev_vp[:])
    eye = v3(*cam.eye[:])
    screen = (f(W), f(H))
    rays = camera_rays_np(cam, W, H)[1]
    for y in range(H):
        for x in range(W):
            d = tuple(rays[y, x])
            h = sc.closest(eye, d, EPS)
            if h is None:  # g_miss: result 0, radiance 0, reproject_uv -1; origin / normal / depth stay 0
                out["position"][y, x] = (0, 0, 0, 1)
                out["normal"][y, x] = (0.5, 0.5, 0.5, 0)
                out["depth"][y, x] = (0, 0, 0, 1)
                out["diffuse"][y, x] = (0, 0, 0, 1)
                out["weight"][y, x] = (-1, -1, 0, 1)
                continue
            k, t, beta, gamma = h
            a = sc.attributes(k, t, beta, gamma, eye, d)
            wsn, wgn = normalize(a["shading"]), normalize(a["geo"])
            ffn = faceforward_neg(wsn, d, wgn)
            hitp = a["front"]
            Kd = sc.kd(k, a["uv"])  # prd.result (1) *= Kd
            depth = length(sub(hitp, eye))
            p = mat_vec(prev_vp, (hitp[0], hitp[1], hitp[2], f(1)))
            iw = f(f(1) / p[3])  # compute_reprojection as g_diffuse.ptx:659-689
            q = tuple(f(fma(f(p[c] * iw), screen[c], screen[c]) * f(0.5)) for c in range(2))
            lp = add(add(sc.light_pos, sc.light_v1), sc.light_v2)
            L = normalize(sub(lp, hitp))
            lit = dot(ffn, L) > 0 and dot(sc.light_n, L) > 0  # the shadow ray's inShadow is never set
            out["position"][y, x] = (*hitp, 1)
            out["normal"][y, x] = (*(fma(c, f(0.5), f(0.5)) for c in wgn), 1.0 if lit else 0.0)
            out["depth"][y, x] = (depth, depth, depth, 1)
            out["diffuse"][y, x] = (*Kd, 1)
            out["weight"][y, x] = (q[0], q[1], 0, 1)
    return out


def shade_np(sc, cam, W, H, frame, spp, mask, weight, history_cache):
    """Entry 3 (fov_path_trace_camera.cu:72-176) for every pixel: (history, shading)."""
    sq = int(np.floor(np.sqrt(spp) + 1e-9))
    assert sq * sq == spp, "the reference's loop covers square spp"
    inv_vp = list(cam.inv_vp[:])
    eye = v3(*cam.eye[:])
    screen = (f(W), f(H))
    js = (f(f(f(1) / screen[0]) / f(sq)), f(f(f(1) / screen[1]) / f(sq)))
    hist = np.zeros((H, W, 4), np.float32)
    shading = np.zeros((H, W, 4), np.float32)
    for v in range(H):
        for u in range(W):
            cw = weight[v, u]
            ch = np.zeros(4, np.float32)
            if cw[2] > 0:
                ch = history_cache[_round_u32(cw[1]), _round_u32(cw[0])].astype(np.float32)
            if not mask[v, u]:
                hist[v, u] = ch
                shading[v, u] = _color_to_accumulated(ch)
                continue
            result = v3(0, 0, 0)
            for s in range(spp, 0, -1):
                rng = Rng(tea16(W * v + u, frame if ch[3] > 0 else 0))
                pixel = (fma(f(f(u) / screen[0]), f(2), f(-1)), fma(f(f(v) / screen[1]), f(2), f(-1)))
                jx = f(f(s % sq) - rng.rnd())
                jy = f(f(s // sq) - rng.rnd())
                dd = (fma(jx, js[0], pixel[0]), fma(jy, js[1], pixel[1]))  # fov_path_trace_camera.ptx:525-528
                tmp = mat_vec(inv_vp, (dd[0], dd[1], f(-1), f(1)))
                d = normalize(sub(div_w(tmp), eye))
                prd = dict(result=v3(0, 0, 0), depth=0, seed=rng.seed, done=False, importance=f(1),
                           reflectance=v3(1, 1, 1))
                trace_radiance(sc, eye, d, prd)
                result = add(result, prd["result"])
            result = scale(result, f(f(1) / f(sq * sq)))
            tm = tonemap(result)
            final = np.array([f(tm[0] + ch[0]), f(tm[1] + ch[1]), f(tm[2] + ch[2]), f(f(1) + ch[3])], np.float32)
            hist[v, u] = final
            shading[v, u] = _color_to_accumulated(final)
    return {"history": hist, "shading": shading}
