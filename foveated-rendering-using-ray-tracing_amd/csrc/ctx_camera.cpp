// ctx_camera.cpp — the camera calls of include/fovrt.h: glm-compatible math (FR/Camera.cpp; glm 0.9.x,
// GLM_FORCE_RADIANS), and the homography between two poses that a warped present takes
// (fr_present_warp_from_poses). Pure host code: no context, no device.
#include <algorithm>
#include <cmath>

#include "../../include/fovrt.h"
#include "scene.h"

using namespace fr;

namespace {
struct Q { float w, x, y, z; };
f3 qrot(Q q, f3 v) {  // glm::operator*(quat, vec3)
  f3 qv = mk3(q.x, q.y, q.z);
  f3 uv = cross(qv, v);
  f3 uuv = cross(qv, uv);
  return v + ((uv * q.w) + uuv) * 2.0f;
}
Q quat_cast(const float m[3][3]) {  // glm::quat_cast(mat3), m[col][row]
  float fx = m[0][0] - m[1][1] - m[2][2];
  float fy = m[1][1] - m[0][0] - m[2][2];
  float fz = m[2][2] - m[0][0] - m[1][1];
  float fw = m[0][0] + m[1][1] + m[2][2];
  int bi = 0;
  float fb = fw;
  if (fx > fb) { fb = fx; bi = 1; }
  if (fy > fb) { fb = fy; bi = 2; }
  if (fz > fb) { fb = fz; bi = 3; }
  float bv = sqrtf(fb + 1.0f) * 0.5f;
  float mult = 0.25f / bv;
  switch (bi) {
    case 0: return Q{bv, (m[1][2] - m[2][1]) * mult, (m[2][0] - m[0][2]) * mult, (m[0][1] - m[1][0]) * mult};
    case 1: return Q{(m[1][2] - m[2][1]) * mult, bv, (m[0][1] + m[1][0]) * mult, (m[2][0] + m[0][2]) * mult};
    case 2: return Q{(m[2][0] - m[0][2]) * mult, (m[0][1] + m[1][0]) * mult, bv, (m[1][2] + m[2][1]) * mult};
    default: return Q{(m[0][1] - m[1][0]) * mult, (m[2][0] + m[0][2]) * mult, (m[1][2] + m[2][1]) * mult, bv};
  }
}
Q qnormalize(Q q) {
  float len = sqrtf(q.w * q.w + q.x * q.x + q.y * q.y + q.z * q.z);
  if (len <= 0.0f) return Q{1, 0, 0, 0};
  float inv = 1.0f / len;
  return Q{q.w * inv, q.x * inv, q.y * inv, q.z * inv};
}
// column-major glm mat4 helpers: M[c][r]
struct M4 { float m[4][4]; };
M4 glm_lookat(f3 eye, f3 center, f3 up) {
  f3 f = normalize(center - eye);
  f3 s = normalize(cross(f, up));
  f3 u = cross(s, f);
  M4 r = {};
  r.m[0][0] = s.x; r.m[1][0] = s.y; r.m[2][0] = s.z;
  r.m[0][1] = u.x; r.m[1][1] = u.y; r.m[2][1] = u.z;
  r.m[0][2] = -f.x; r.m[1][2] = -f.y; r.m[2][2] = -f.z;
  r.m[3][0] = -dot(s, eye); r.m[3][1] = -dot(u, eye); r.m[3][2] = dot(f, eye);
  r.m[3][3] = 1.0f;
  return r;
}
M4 glm_perspective(float fovy, float aspect, float zn, float zf) {
  float t = tanf(fovy / 2.0f);
  M4 r = {};
  r.m[0][0] = 1.0f / (aspect * t);
  r.m[1][1] = 1.0f / t;
  r.m[2][2] = -(zf + zn) / (zf - zn);
  r.m[2][3] = -1.0f;
  r.m[3][2] = -(2.0f * zf * zn) / (zf - zn);
  return r;
}
M4 glm_mul(const M4& a, const M4& b) {  // glm mat4 * mat4
  M4 r;
  for (int c = 0; c < 4; c++)
    for (int k = 0; k < 4; k++)
      r.m[c][k] = a.m[0][k] * b.m[c][0] + a.m[1][k] * b.m[c][1] + a.m[2][k] * b.m[c][2] + a.m[3][k] * b.m[c][3];
  return r;
}
void pose_matrices(const fr_camera_pose* p, M4& V, M4& P) {
  Q q{p->rot[0], p->rot[1], p->rot[2], p->rot[3]};
  f3 pos = mk3(p->pos[0], p->pos[1], p->pos[2]);
  f3 front = qrot(q, mk3(0, 0, -1));
  f3 upv = qrot(q, mk3(0, 1, 0));
  V = glm_lookat(pos, pos + front, upv);
  P = glm_perspective(p->fovy_deg * 0.01745329251994329576923690768489f, p->aspect, p->znear, p->zfar);
}
void to_rowmajor(const M4& a, float out[16]) {
  for (int r = 0; r < 4; r++)
    for (int c = 0; c < 4; c++) out[r * 4 + c] = a.m[c][r];
}
template <class T>
bool invert_rowmajor(const T in[16], T out[16]) {  // Gauss-Jordan in f64, rounded once
  double a[4][8];
  for (int r = 0; r < 4; r++)
    for (int c = 0; c < 8; c++) a[r][c] = c < 4 ? (double)in[r * 4 + c] : (c - 4 == r ? 1.0 : 0.0);
  for (int c = 0; c < 4; c++) {
    int piv = c;
    for (int r = c + 1; r < 4; r++) if (fabs(a[r][c]) > fabs(a[piv][c])) piv = r;
    if (a[piv][c] == 0.0) return false;
    if (piv != c) for (int k = 0; k < 8; k++) std::swap(a[c][k], a[piv][k]);
    double d = a[c][c];
    for (int k = 0; k < 8; k++) a[c][k] /= d;
    for (int r = 0; r < 4; r++) {
      if (r == c) continue;
      double f = a[r][c];
      for (int k = 0; k < 8; k++) a[r][k] -= f * a[c][k];
    }
  }
  for (int r = 0; r < 4; r++)
    for (int c = 0; c < 4; c++) out[r * 4 + c] = (T)a[r][c + 4];
  return true;
}
// proj * view of a pose, row-major, the fp32 matrices of fr_camera_matrices multiplied in f64
void pose_pv_f64(const fr_camera_pose* p, double out[16]) {
  M4 V, P;
  pose_matrices(p, V, P);
  for (int r = 0; r < 4; r++)
    for (int c = 0; c < 4; c++) {
      double s = 0.0;
      for (int k = 0; k < 4; k++) s += (double)P.m[k][r] * (double)V.m[c][k];
      out[r * 4 + c] = s;
    }
}

}  // namespace

extern "C" {

int fr_preset_camera(int scene, float eye[3], float target[3]) {
  f3 e, t;
  preset_camera(scene, e, t);
  eye[0] = e.x; eye[1] = e.y; eye[2] = e.z;
  target[0] = t.x; target[1] = t.y; target[2] = t.z;
  return FR_OK;
}

int fr_camera_look_at(fr_camera_pose* pose, const float target[3], const float up[3]) {
  if (!pose || !target) return FR_E_INVALID;
  f3 pos = mk3(pose->pos[0], pose->pos[1], pose->pos[2]);
  f3 tg = mk3(target[0], target[1], target[2]);
  f3 u = up ? mk3(up[0], up[1], up[2]) : mk3(0, 1, 0);
  f3 z = normalize(pos - tg);
  f3 x = normalize(cross(u, z));
  f3 y = normalize(cross(z, x));
  float m[3][3] = {{x.x, x.y, x.z}, {y.x, y.y, y.z}, {z.x, z.y, z.z}};
  Q q = qnormalize(quat_cast(m));
  pose->rot[0] = q.w; pose->rot[1] = q.x; pose->rot[2] = q.y; pose->rot[3] = q.z;
  return FR_OK;
}

int fr_camera_matrices(const fr_camera_pose* pose, float view[16], float proj[16]) {
  if (!pose) return FR_E_INVALID;
  M4 V, P;
  pose_matrices(pose, V, P);
  if (view) to_rowmajor(V, view);
  if (proj) to_rowmajor(P, proj);
  return FR_OK;
}

int fr_camera_uniforms(const fr_camera_pose* cur, const fr_camera_pose* prev, int width, int height, fr_camera* out) {
  if (!cur || !out || width <= 0 || height <= 0) return FR_E_INVALID;
  if (!prev) prev = cur;
  M4 V, P, PV, pV, pP, pPV;
  pose_matrices(cur, V, P);
  PV = glm_mul(P, V);
  pose_matrices(prev, pV, pP);
  pPV = glm_mul(pP, pV);
  float rm[16];
  to_rowmajor(PV, rm);
  if (!invert_rowmajor(rm, out->inv_vp)) return FR_E_INVALID;
  to_rowmajor(pPV, out->prev_vp);
  for (int k = 0; k < 3; k++) { out->eye[k] = cur->pos[k]; out->prev_eye[k] = prev->pos[k]; }
  Q q{cur->rot[0], cur->rot[1], cur->rot[2], cur->rot[3]};
  f3 up = qrot(q, mk3(0, 1, 0));
  out->up[0] = up.x; out->up[1] = up.y; out->up[2] = up.z;
  f3 fr = qrot(q, mk3(0, 0, -1));
  out->target[0] = cur->pos[0] + fr.x; out->target[1] = cur->pos[1] + fr.y; out->target[2] = cur->pos[2] + fr.z;
  // g_gaze = (w/2, h/2) ints (FR/gui.cpp:34-35); gaze = (g_gaze.x, H - g_gaze.y) (FR/PathTracer.cpp:795)
  out->gaze[0] = (float)(width / 2);
  out->gaze[1] = (float)(height - height / 2);
  return FR_OK;
}

// The homography of a late reprojection (include/fovrt.h, "Present"): output texel centres of the display camera's
// viewport to source texel coordinates of the rendered camera's image, through the points at one NDC depth of the
// display camera. f64 from the fp32 matrices of fr_camera_matrices on, rounded once at the end.
int fr_present_warp_from_poses(const fr_camera_pose* rendered, const fr_camera_pose* display, int width, int height,
                               int out_width, int out_height, float ndc_depth, fr_present_warp* warp) {
  if (!rendered || !display || !warp) return FR_E_INVALID;
  for (int v : {width, height, out_width, out_height}) if (v < 1 || v > 32767) return FR_E_INVALID;
  if (!std::isfinite(ndc_depth)) return FR_E_INVALID;
  double Mr[16], Md[16], inv[16];
  pose_pv_f64(rendered, Mr);
  pose_pv_f64(display, Md);
  for (int k = 0; k < 16; k++) if (!std::isfinite(Mr[k]) || !std::isfinite(Md[k])) return FR_E_INVALID;
  if (!invert_rowmajor(Md, inv)) return FR_E_INVALID;
  // A = M_r M_d^-1, formed as I + (M_r - M_d) M_d^-1: the identity exactly for equal poses
  double A[16];
  for (int r = 0; r < 4; r++)
    for (int c = 0; c < 4; c++) {
      double s = 0.0;
      for (int k = 0; k < 4; k++) s += (Mr[r * 4 + k] - Md[r * 4 + k]) * inv[k * 4 + c];
      A[r * 4 + c] = (r == c ? 1.0 : 0.0) + s;
    }
  // The rendered camera's clip coordinate i of the display camera's NDC point (nx, ny, z, 1), nx = 2 px / ow - 1:
  // (2 A_i0 / ow) px + (2 A_i1 / oh) py + (A_i2 z + A_i3 - A_i0 - A_i1). Source texel x = (clip_x / clip_w + 1) W / 2 =
  // (clip_x + clip_w) (W / 2) / clip_w, the same for y; W / ow is formed by one division, so equal sizes give 1.
  const double z = (double)ndc_depth, W = width, H = height, ow = out_width, oh = out_height;
  double cx[3], cy[3], cw[3];
  const auto clip_row = [&A, z](int i, double g[3]) {
    g[0] = A[i * 4];
    g[1] = A[i * 4 + 1];
    g[2] = A[i * 4 + 2] * z + A[i * 4 + 3] - A[i * 4] - A[i * 4 + 1];
  };
  clip_row(0, cx); clip_row(1, cy); clip_row(3, cw);
  const double g[9] = {(cx[0] + cw[0]) * W / ow, (cx[1] + cw[1]) * W / oh, (cx[2] + cw[2]) * W / 2.0,
                       (cy[0] + cw[0]) * H / ow, (cy[1] + cw[1]) * H / oh, (cy[2] + cw[2]) * H / 2.0,
                       cw[0] * 2.0 / ow,         cw[1] * 2.0 / oh,         cw[2]};
  for (double v : g) if (!std::isfinite(v)) return FR_E_INVALID;
  // g[8] is clip w at output corner (0, 0): it must be positive (in front of the rendered camera's eye plane) and not
  // lost against the change of w across the output
  const double span = std::max(std::max(fabs(g[6]) * ow, fabs(g[7]) * oh), fabs(g[8]));
  if (!(g[8] > span * (1.0 / 1048576.0))) return FR_E_INVALID;
  fr_present_warp out;
  for (int k = 0; k < 9; k++) {
    out.h[k] = (float)(g[k] / g[8]);
    if (!std::isfinite(out.h[k])) return FR_E_INVALID;
  }
  out.out_width = out_width;
  out.out_height = out_height;
  *warp = out;
  return FR_OK;
}

// The reprojected present's parameters for the same two poses: vp, the display camera's proj * view (the fp32 matrices
// of fr_camera_matrices multiplied in f64, rounded once), and the homography above for the places nothing reaches.
int fr_present_reproject_from_poses(const fr_camera_pose* rendered, const fr_camera_pose* display, int width, int height,
                                    int out_width, int out_height, float ndc_depth, fr_present_reproject* rp) {
  if (!rp) return FR_E_INVALID;
  fr_present_reproject out;
  if (int rc = fr_present_warp_from_poses(rendered, display, width, height, out_width, out_height, ndc_depth, &out.fallback))
    return rc;
  double Md[16];
  pose_pv_f64(display, Md);  // (finite: the warp checked it)
  for (int k = 0; k < 16; k++) {
    out.vp[k] = (float)Md[k];
    if (!std::isfinite(out.vp[k])) return FR_E_INVALID;
  }
  *rp = out;
  return FR_OK;
}

}  // extern "C"
