// vc_register.hpp -- the arithmetic of depth registration, shared by the kernels (vc_register.hip), the host entry points and the host
// harness of the CPU tests: a depth pixel of the source camera S placed at its measured distance, taken into the destination camera D
// (p_d = R p_s + t) and projected there; the rectangle of destination pixels it lands on; the key of the depth test; the visibility test
// of the colour gather.  All projection goes through project_any (vc_math.hpp) and undist_unproject (vc_undistort.hpp: Newton inversion,
// all six models); nothing here restates a camera formula.  Definitions and drop rules: include/vicalib_amd.h.
#pragma once
#include "vc_rectify.hpp"

namespace vc {

enum { kRegKindZ = 0, kRegKindRange = 1 };
enum { kRegNearest = 0, kRegFootprint = 1 };
// the eight counters: the rule that dropped a source pixel (0-5), candidates that reached the depth test, destination pixels filled
enum { kRegDropZero = 0, kRegDropNoRay = 1, kRegDropBehind = 2, kRegDropOutside = 3, kRegDropValue = 4, kRegDropFootprint = 5, kRegCandidates = 6, kRegFilled = 7,
       kRegCounters = 8 };
constexpr int kRegMaxFootprint = 8;                        // destination pixels in x or y before clipping
constexpr unsigned long long kRegEmptyKey = ~0ull;         // what the key buffer is cleared to: larger than every candidate's key

struct RegCam {
  int model, w, h, pad_;
  double K[10];
  ModelPre pre;
};
struct RegisterPlan {
  RegCam s, d;
  double R[9], t[3];               // p_d = R p_s + t (row-major)
  double unit_src, unit_dst;       // metres per count
  int kind, splat;
};
struct RegRect { int x0, x1, y0, y1; };      // closed, clipped to D's image

inline bool reg_args_ok(double unit_src, double unit_dst, int kind, int splat) {
  return std::isfinite(unit_src) && std::isfinite(unit_dst) && unit_src > 0.0 && unit_dst > 0.0 && (kind == kRegKindZ || kind == kRegKindRange) &&
         (splat == kRegNearest || splat == kRegFootprint);
}
inline void reg_cam_fill(RegCam* c, int model, const double* params, int nparams, int w, int h) {
  c->model = model; c->w = w; c->h = h; c->pad_ = 0;
  for (int k = 0; k < 10; ++k) c->K[k] = k < nparams ? params[k] : 0.0;
  model_precompute(model, c->K, &c->pre);
}
// the pair relation of the rectifier (vc_rectify.hpp) from two poses that pose_ok has normalised
inline void reg_relative_pose(const double* T_ck_s, const double* T_ck_d, double* R, double* t) {
  double Rs[9], Rd[9];
  quat_to_R(T_ck_s, Rs); quat_to_R(T_ck_d, Rd);
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) R[3 * i + j] = Rd[3 * i] * Rs[3 * j] + Rd[3 * i + 1] * Rs[3 * j + 1] + Rd[3 * i + 2] * Rs[3 * j + 2];
  for (int i = 0; i < 3; ++i) t[i] = T_ck_d[4 + i] - (R[3 * i] * T_ck_s[4] + R[3 * i + 1] * T_ck_s[5] + R[3 * i + 2] * T_ck_s[6]);
}

// the ray of source position (u, v); false = rule 1: the inversion failed, or r_z <= 0 under kind Z
VC_HD bool reg_ray(const RegisterPlan& p, double u, double v, double* ray) {
  if (!undist_unproject(p.s.model, p.s.K, p.s.pre, u, v, ray)) return false;
  return p.kind != kRegKindZ || ray[2] > 0.0;
}
// the point at measured distance m (metres) on `ray`, in D's frame
VC_HD void reg_transfer(const RegisterPlan& p, const double* ray, double m, double* pd) {
  const double s = p.kind == kRegKindZ ? m / ray[2] : m / sqrt(ray[0] * ray[0] + ray[1] * ray[1] + ray[2] * ray[2]);
  const double ps[3] = {ray[0] * s, ray[1] * s, ray[2] * s};
  for (int i = 0; i < 3; ++i) pd[i] = p.R[3 * i] * ps[0] + p.R[3 * i + 1] * ps[1] + p.R[3 * i + 2] * ps[2] + p.t[i];
}
// ... projected into D and measured there in D's unit, before any rounding; false = rule 2: z <= 0 (not kb4, the undistorter's rule) or
// a projection that is not finite
VC_HD bool reg_project(const RegisterPlan& p, const double* ray, double m, double* q, double* wv) {
  double pd[3];
  reg_transfer(p, ray, m, pd);
  if (!(pd[2] > 0.0) && p.d.model != kKb4) return false;
  project_any<false>(p.d.model, pd, p.d.K, p.d.pre, q, nullptr, nullptr);
  if (!(fabs(q[0]) <= 1e300 && fabs(q[1]) <= 1e300)) return false;
  *wv = (p.kind == kRegKindZ ? pd[2] : sqrt(pd[0] * pd[0] + pd[1] * pd[1] + pd[2] * pd[2])) / p.unit_dst;
  return true;
}

// One source pixel with its centre ray rc and, in footprint mode, the rays ra / rb of its corners (i - 0.5, j - 0.5) and (i + 0.5, j + 0.5):
// the rule that drops it (the first that applies), or kRegCandidates with its value *w and the rectangle of destination pixels it lands on.
VC_HD int reg_candidate(const RegisterPlan& p, unsigned value, const double* rc, bool okc, const double* ra, bool oka, const double* rb, bool okb, unsigned* w,
                        RegRect* rect) {
  if (value == 0) return kRegDropZero;
  const bool fp = p.splat == kRegFootprint;
  if (!okc || (fp && !(oka && okb))) return kRegDropNoRay;
  const double m = (double)value * p.unit_src;
  double q[2], qa[2], qb[2], wv, unused;
  if (!reg_project(p, rc, m, q, &wv)) return kRegDropBehind;
  double x0, x1, y0, y1;
  if (fp) {
    if (!reg_project(p, ra, m, qa, &unused) || !reg_project(p, rb, m, qb, &unused)) return kRegDropBehind;
    x0 = floor(fmin(qa[0], qb[0]) + 0.5); x1 = floor(fmax(qa[0], qb[0]) + 0.5);
    y0 = floor(fmin(qa[1], qb[1]) + 0.5); y1 = floor(fmax(qa[1], qb[1]) + 0.5);
  } else {
    x0 = x1 = floor(q[0] + 0.5); y0 = y1 = floor(q[1] + 0.5);
  }
  const double xm = (double)(p.d.w - 1), ym = (double)(p.d.h - 1);
  if (!(x1 >= 0.0 && x0 <= xm && y1 >= 0.0 && y0 <= ym)) return kRegDropOutside;
  const double wr = floor(wv + 0.5);
  if (!(wr >= 1.0 && wr <= 65535.0)) return kRegDropValue;
  if (fp && (x1 - x0 + 1.0 > (double)kRegMaxFootprint || y1 - y0 + 1.0 > (double)kRegMaxFootprint)) return kRegDropFootprint;
  rect->x0 = (int)fmax(x0, 0.0); rect->x1 = (int)fmin(x1, xm); rect->y0 = (int)fmax(y0, 0.0); rect->y1 = (int)fmin(y1, ym);
  *w = (unsigned)wr;
  return kRegCandidates;
}

// the depth test's key: the smallest wins -- the nearest surface, among equal values the lowest source index
VC_HD unsigned long long reg_key(unsigned w, unsigned src_index) { return ((unsigned long long)w << 32) | (unsigned long long)src_index; }
VC_HD unsigned reg_key_depth(unsigned long long key) { return key == kRegEmptyKey ? 0u : (unsigned)(key >> 32); }
VC_HD int reg_key_index(unsigned long long key) { return key == kRegEmptyKey ? -1 : (int)(unsigned)(key & 0xffffffffull); }

// Colour into depth geometry, first half: source pixel with centre ray rc passes rules 0-2 and its projection lies in D's image under the
// undistorter's border rule -> the (clamped) position, the destination pixel whose depth test decides, and the pixel's own value *wr
VC_HD bool reg_gather_position(const RegisterPlan& p, unsigned value, const double* rc, bool okc, double* x, double* y, int* pix, double* wr) {
  if (value == 0 || !okc) return false;
  double q[2], wv;
  if (!reg_project(p, rc, (double)value * p.unit_src, q, &wv)) return false;
  const double xm = (double)(p.d.w - 1), ym = (double)(p.d.h - 1);
  if (!(q[0] >= -kUndistBorderTol && q[0] <= xm + kUndistBorderTol && q[1] >= -kUndistBorderTol && q[1] <= ym + kUndistBorderTol)) return false;
  *x = fmin(fmax(q[0], 0.0), xm);
  *y = fmin(fmax(q[1], 0.0), ym);
  *pix = (int)floor(*y + 0.5) * p.d.w + (int)floor(*x + 0.5);
  *wr = floor(wv + 0.5);
  return true;
}
// ... second half: the pixel is no further than occl_tol behind what won the depth test there
VC_HD bool reg_visible(double wr, unsigned long long key, double occl_tol) { return key != kRegEmptyKey && wr <= (double)(unsigned)(key >> 32) + occl_tol; }

// the bilinear rule of vc_undistort_images at (x, y) inside [0, w - 1] x [0, h - 1], unrounded
VC_HD double reg_bilinear(const unsigned char* img, int pitch, int w, int h, double x, double y) {
  const int x0 = (int)fmin(floor(x), (double)(w - 2)), y0 = (int)fmin(floor(y), (double)(h - 2));
  const double ax = x - (double)x0, ay = y - (double)y0;
  const unsigned char* r0 = img + (size_t)y0 * pitch + x0;
  return (1.0 - ay) * ((1.0 - ax) * (double)r0[0] + ax * (double)r0[1]) + ay * ((1.0 - ax) * (double)r0[pitch] + ax * (double)r0[pitch + 1]);
}

// the continuous face: (u, v, value) at any sub-pixel position -> (q_x, q_y, m_d / unit_dst); false: rule 1 or 2, or a value that is not
// positive and finite
VC_HD bool reg_point(const RegisterPlan& p, double u, double v, double value, double* out) {
  if (!(value > 0.0 && value <= 1e300)) return false;
  double ray[3];
  if (!reg_ray(p, u, v, ray)) return false;
  return reg_project(p, ray, value * p.unit_src, out, out + 2);
}

}  // namespace vc
