// vc_compare.hpp -- the arithmetic of comparing two calibrations of one camera in pixel space, shared by the kernels (vc_compare.hip), the host
// entry points and the host harness of the CPU tests.  For every sample q of a lattice over the image: unproject q with calibration A
// (undist_unproject, vc_undistort.hpp), rotate the ray by R, project it with calibration B (project_any, vc_math.hpp) and ask how far from q
// it lands: d = project(B, R a) - q.  R is either given or the IMPLIED rotation: the one the extrinsics would absorb, fitted by Gauss-Newton
// on sum |d|^2 over the samples inside a radius, started from Horn's rotation (rigid_rotation, vc_rectify.hpp) of the two ray bundles.
// Nothing here restates a camera formula.
#pragma once
#include "vc_rectify.hpp"

namespace vc {

constexpr int kCmpMaxSamples = 1 << 22;
constexpr int kCmpMaxRings = 64;
constexpr int kCmpDefaultRings = 8;            // the ring count the difference sweep bins at; any other is a rings-only sweep
constexpr int kCmpDefaultIters = 20, kCmpMaxIters = 100, kCmpMaxHalvings = 8;
constexpr double kCmpStepTol = 1e-9;           // rad: below 3.5e-7 px wherever f (1 + r_u^2) <= 3500
enum { kCmpFlagA = 1, kCmpFlagB = 2, kCmpFlagInvalid = 4 };
enum { kCmpConverged = 0, kCmpMaxItersReached = 1, kCmpNoDecrease = 2 };
// one fit sweep's sums: J^T J (xx xy xz yy yz zz), J^T d (3), E, samples used, samples of the fit set left out at this R
constexpr int kCmpFitDoubles = 12;
// the difference sweep's summary: count, invalid, sum du, sum dv, sum |d|^2, max |d|^2, its sample; then per ring count, invalid, sum |d|^2, max |d|^2
constexpr int kCmpSumDoubles = 7, kCmpRingDoubles = 4;

struct CmpPlan {
  int model_a, model_b, w, h, gx, gy, n, pad_;
  double Ka[10], Kb[10];
  ModelPre pre_a, pre_b;
};
// the one check of a lattice over a w x h image
inline bool cvt_grid_ok(int w, int h, int gx, int gy) { return gx >= 2 && gy >= 2 && gx <= w && gy <= h && (long long)gx * gy <= kCmpMaxSamples; }
// the plan of cameras A and B on a gx x gy lattice over their w x h image (a tool with one camera gives it as B too)
inline void cmp_plan_set(CmpPlan* p, int model_a, const double* Ka, int nka, int model_b, const double* Kb, int nkb, int w, int h, int gx, int gy) {
  *p = CmpPlan{};
  p->model_a = model_a; p->model_b = model_b; p->w = w; p->h = h; p->gx = gx; p->gy = gy; p->n = gx * gy;
  for (int k = 0; k < nka; ++k) p->Ka[k] = Ka[k];
  for (int k = 0; k < nkb; ++k) p->Kb[k] = Kb[k];
  model_precompute(model_a, p->Ka, &p->pre_a); model_precompute(model_b, p->Kb, &p->pre_b);
}

// x * x + y * y with both products rounded (no fused multiply-add): the same bits on the device, on the host and in numpy, so that a
// maximum over |d|^2 can be compared exactly
VC_HD double cmp_norm2(double x, double y) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const double a = x * x, b = y * y;
  return a + b;
}
// sample s = j gx + i sits at q = (i (w - 1) / (gx - 1), j (h - 1) / (gy - 1)); rho = |q - c| / |c| with c the image centre
VC_HD void cmp_sample(const CmpPlan& p, int s, double* qx, double* qy, double* rho) {
  const int j = s / p.gx, i = s - j * p.gx;
  *qx = (double)(i * (p.w - 1)) / (double)(p.gx - 1);
  *qy = (double)(j * (p.h - 1)) / (double)(p.gy - 1);
  const double cx = 0.5 * (double)(p.w - 1), cy = 0.5 * (double)(p.h - 1);
  *rho = sqrt(cmp_norm2(*qx - cx, *qy - cy)) / sqrt(cmp_norm2(cx, cy));
}
VC_HD int cmp_ring(double rho, int n_rings) {
  const int k = (int)(rho * (double)n_rings);
  return k < n_rings - 1 ? k : n_rings - 1;
}
// both inversions of one sample: a and b of unit length; the flags' bits 0 (A failed) and 1 (B failed).  A failed side's ray is zero.
VC_HD int cmp_rays(const CmpPlan& p, double qx, double qy, double* a, double* b) {
  int flags = 0;
  if (!undist_unproject(p.model_a, p.Ka, p.pre_a, qx, qy, a)) { flags |= kCmpFlagA; a[0] = a[1] = a[2] = 0.0; }
  else { const double in = 1.0 / sqrt(a[0] * a[0] + a[1] * a[1] + a[2] * a[2]); a[0] *= in; a[1] *= in; a[2] *= in; }
  if (!undist_unproject(p.model_b, p.Kb, p.pre_b, qx, qy, b)) { flags |= kCmpFlagB; b[0] = b[1] = b[2] = 0.0; }
  else { const double in = 1.0 / sqrt(b[0] * b[0] + b[1] * b[1] + b[2] * b[2]); b[0] *= in; b[1] *= in; b[2] *= in; }
  return flags;
}
// d = project(B, R a) - q of a sample whose inversions both succeeded; false: (R a)_z <= 0 (not kb4) or d is not finite
template <bool JAC>
VC_HD bool cmp_project(const CmpPlan& p, const double* R, const double* a, double qx, double qy, double* ra, double* d, double* A) {
  ra[0] = R[0] * a[0] + R[1] * a[1] + R[2] * a[2];
  ra[1] = R[3] * a[0] + R[4] * a[1] + R[5] * a[2];
  ra[2] = R[6] * a[0] + R[7] * a[1] + R[8] * a[2];
  if (!(ra[2] > 0.0) && p.model_b != kKb4) return false;
  double pix[2], B[20];
  project_any<JAC>(p.model_b, ra, p.Kb, p.pre_b, pix, A, B);
  d[0] = pix[0] - qx; d[1] = pix[1] - qy;
  return fabs(d[0]) <= 1e300 && fabs(d[1]) <= 1e300;         // (a NaN fails the comparison)
}
VC_HD bool cmp_diff_sample(const CmpPlan& p, const double* R, const double* a, double qx, double qy, double* d) {
  double ra[3];
  return cmp_project<false>(p, R, a, qx, qy, ra, d, nullptr);
}
// One sample of a fit sweep at R, with the left perturbation R <- exp(w) R: the rows J = -A [R a]x (2 x 3) and d are added to
// acc = [J^T J: xx xy xz yy yz zz | J^T d (3) | |d|^2].  false (acc untouched): the sample is invalid at this R and is left out.
// Every index is a constant: the ten sums stay in registers.
VC_HD bool cmp_fit_sample(const CmpPlan& p, const double* R, const double* a, double qx, double qy, double* acc) {
  double ra[3], d[2], A[6];
  if (!cmp_project<true>(p, R, a, qx, qy, ra, d, A)) return false;
  const double x = ra[0], y = ra[1], z = ra[2];
  // A [v]x with [v]x = [0 -z y; z 0 -x; -y x 0]
  const double j00 = -(A[1] * z - A[2] * y), j01 = -(A[2] * x - A[0] * z), j02 = -(A[0] * y - A[1] * x);
  const double j10 = -(A[4] * z - A[5] * y), j11 = -(A[5] * x - A[3] * z), j12 = -(A[3] * y - A[4] * x);
  acc[0] += j00 * j00 + j10 * j10; acc[1] += j00 * j01 + j10 * j11; acc[2] += j00 * j02 + j10 * j12;
  acc[3] += j01 * j01 + j11 * j11; acc[4] += j01 * j02 + j11 * j12; acc[5] += j02 * j02 + j12 * j12;
  acc[6] += j00 * d[0] + j10 * d[1]; acc[7] += j01 * d[0] + j11 * d[1]; acc[8] += j02 * d[0] + j12 * d[1];
  acc[9] += d[0] * d[0] + d[1] * d[1];
  return true;
}

// ---- host side of the fit: the same driver for the device sweeps and for the host harness -----------------------------------------
// w = -S^-1 g for the symmetric S = [xx xy xz yy yz zz] by LDL^T; false: a pivot that is not positive
inline bool cmp_solve_step(const double* S, const double* g, double* w) {
  const double d0 = S[0];
  if (!(d0 > 0.0)) return false;
  const double l10 = S[1] / d0, l20 = S[2] / d0;
  const double d1 = S[3] - l10 * S[1];
  if (!(d1 > 0.0)) return false;
  const double l21 = (S[4] - l20 * S[1]) / d1;
  const double d2 = S[5] - l20 * S[2] - l21 * l21 * d1;
  if (!(d2 > 0.0)) return false;
  const double y0 = -g[0], y1 = -g[1] - l10 * y0, y2 = -g[2] - l20 * y0 - l21 * y1;
  w[2] = y2 / d2;
  w[1] = y1 / d1 - l21 * w[2];
  w[0] = y0 / d0 - l10 * w[1] - l20 * w[2];
  return w[0] == w[0] && w[1] == w[1] && w[2] == w[2];
}
// out = exp(w) R
inline void cmp_rotate_left(const double* w, const double* R, double* out) {
  double q[4], E[9];
  so3_exp(w, q);
  const double in = 1.0 / sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
  for (int k = 0; k < 4; ++k) q[k] *= in;
  quat_to_R(q, E);
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) out[3 * i + j] = E[3 * i] * R[j] + E[3 * i + 1] * R[3 + j] + E[3 * i + 2] * R[6 + j];
}
struct CmpFit {
  double R[9];
  int status, iterations;
  long long n_fit, n_left_out;
  double cost0, cost;
};
// Gauss-Newton on E(R) = sum over the fit set of |d(R)|^2 from R0.  eval(R, sums) fills the kCmpFitDoubles sums of one sweep at R and returns
// 0, or a status that ends the fit and is handed on.  A step that does not lower E is halved, up to kCmpMaxHalvings times; when no trial
// lowers E the fit ends with kCmpNoDecrease at the last accepted R.  A Gauss-Newton step of |w| <= kCmpStepTol ends the fit as converged: it
// is taken if it lowers E and dropped otherwise (at that size E's own rounding decides which; no pixel moves by 3.5e-7 px either way), and
// it is not halved.  Returns 0, -1 (a 3 x 3 system without a positive pivot) or eval's status.
template <class Eval>
inline int cmp_gauss_newton(Eval&& eval, const double* R0, int max_iters, CmpFit* f) {
  const int cap = max_iters <= 0 ? kCmpDefaultIters : max_iters > kCmpMaxIters ? kCmpMaxIters : max_iters;
  double cur[kCmpFitDoubles], trial[kCmpFitDoubles], Rt[9];
  for (int k = 0; k < 9; ++k) f->R[k] = R0[k];
  int rc = eval(f->R, cur);
  if (rc != 0) return rc;
  f->cost0 = cur[9];
  f->status = kCmpMaxItersReached; f->iterations = 0;
  while (f->iterations < cap) {
    double w[3];
    if (!cmp_solve_step(cur, cur + 6, w)) return -1;
    const bool last = sqrt(w[0] * w[0] + w[1] * w[1] + w[2] * w[2]) <= kCmpStepTol;
    bool accepted = false;
    for (int h = 0; h <= (last ? 0 : kCmpMaxHalvings); ++h) {
      cmp_rotate_left(w, f->R, Rt);
      if ((rc = eval(Rt, trial)) != 0) return rc;
      if (trial[9] < cur[9]) { accepted = true; break; }
      for (int k = 0; k < 3; ++k) w[k] *= 0.5;
    }
    if (accepted) {
      for (int k = 0; k < 9; ++k) f->R[k] = Rt[k];
      for (int k = 0; k < kCmpFitDoubles; ++k) cur[k] = trial[k];
      ++f->iterations;
    }
    if (last) { f->status = kCmpConverged; break; }
    if (!accepted) { f->status = kCmpNoDecrease; break; }
  }
  f->cost = cur[9];
  f->n_left_out = (long long)cur[11];
  return 0;
}

// ---- extrinsics (host): camera c against camera 0 of two rigs A and B, p_c = R_rel p_0 + t_rel from each rig's T_ck --------------------
inline void cmp_relative(const double* T0, const double* Tc, double* R, double* c) {
  double R0[9], Rc[9], t[3];
  quat_to_R(T0, R0); quat_to_R(Tc, Rc);
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) R[3 * i + j] = Rc[3 * i] * R0[3 * j] + Rc[3 * i + 1] * R0[3 * j + 1] + Rc[3 * i + 2] * R0[3 * j + 2];
  for (int i = 0; i < 3; ++i) t[i] = Tc[4 + i] - (R[3 * i] * T0[4] + R[3 * i + 1] * T0[5] + R[3 * i + 2] * T0[6]);
  for (int i = 0; i < 3; ++i) c[i] = -(R[i] * t[0] + R[3 + i] * t[1] + R[6 + i] * t[2]);
}
inline double cmp_rotation_angle(const double* M) {
  const double vx = M[7] - M[5], vy = M[2] - M[6], vz = M[3] - M[1];
  return atan2(0.5 * sqrt(vx * vx + vy * vy + vz * vz), 0.5 * (M[0] + M[4] + M[8] - 1.0));
}
// out = [angle of R_rel_B^T R_c R_rel_A R_0^T, |c_B - R_0 c_A|] with c_X = -R_rel_X^T t_rel_X
inline void cmp_extrinsics(const double* Ta0, const double* Tac, const double* Tb0, const double* Tbc, const double* R_0, const double* R_c, double* out) {
  double Ra[9], ca[3], Rb[9], cb[3], M1[9], M2[9], M3[9];
  cmp_relative(Ta0, Tac, Ra, ca); cmp_relative(Tb0, Tbc, Rb, cb);
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) M1[3 * i + j] = R_c[3 * i] * Ra[j] + R_c[3 * i + 1] * Ra[3 + j] + R_c[3 * i + 2] * Ra[6 + j];               // R_c R_rel_A
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) M2[3 * i + j] = M1[3 * i] * R_0[3 * j] + M1[3 * i + 1] * R_0[3 * j + 1] + M1[3 * i + 2] * R_0[3 * j + 2];      // ... R_0^T
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) M3[3 * i + j] = Rb[i] * M2[j] + Rb[3 + i] * M2[3 + j] + Rb[6 + i] * M2[6 + j];                           // R_rel_B^T ...
  out[0] = cmp_rotation_angle(M3);
  double e[3];
  for (int i = 0; i < 3; ++i) e[i] = cb[i] - (R_0[3 * i] * ca[0] + R_0[3 * i + 1] * ca[1] + R_0[3 * i + 2] * ca[2]);
  out[1] = sqrt(e[0] * e[0] + e[1] * e[1] + e[2] * e[2]);
}

}  // namespace vc
