// vc_rectify.hpp -- the arithmetic of stereo rectification and of the stereo consistency check, shared by the kernel (vc_rectify.hip), the
// host entry points and the host harness of the CPU tests: the rectifying rotations of two calibrated cameras, one matched corner pair
// (row misalignment, disparity, triangulated point) and the small dense part of the rigid fit of the triangulated corners onto the target
// (Horn's quaternion method).  Cameras go through vc_undistort.hpp (undist_point: Newton inversion, R_ds, pinhole); nothing here restates
// a camera formula.
//
// Conventions (include/vicalib_amd.h): p_c = R_ck p_k + t_ck.  For cameras a and b: R = R_bk R_ak^T, t = t_bk - R t_ak, p_b = R p_a + t,
// and the centre of b in a's frame is c = -R^T t.
#pragma once
#include "vc_undistort.hpp"

namespace vc {

enum { kRectOk = 0, kRectCoincident = 1, kRectVertical = 2 };
constexpr double kRectMinBaseline = 1e-9;      // |c| below this: the two centres coincide
constexpr int kRectPairDoubles = 6;            // per pair: dv, d, P (3), v = (va + vb) / 2
constexpr int kRectJacobiSweeps = 8;           // cyclic sweeps over the 4 x 4 matrix: quadratic convergence, rounding level after 5

// both sides of a rectifier as the kernel sees them: the same destination pinhole camera (dl) in both plans
struct RectPlan {
  UndistPlan a, b;
  double baseline;          // signed: e1 . c
};

// a finite pose whose quaternion has unit length to 1e-6, normalised (host: what the entry points hold a caller's T_ck to)
inline bool pose_ok(const double* T, double* out) {
  if (!T) return false;
  for (int k = 0; k < 7; ++k) if (!std::isfinite(T[k])) return false;
  const double n = std::sqrt(T[0] * T[0] + T[1] * T[1] + T[2] * T[2] + T[3] * T[3]);
  if (!(std::fabs(n - 1.0) <= 1e-6)) return false;
  for (int k = 0; k < 4; ++k) out[k] = T[k] / n;
  for (int k = 4; k < 7; ++k) out[k] = T[k];
  return true;
}

// Rotations of the two cameras into the common rectified frame (rows e1 e2 e3 of R_ds_a; R_ds_b = R_ds_a R^T):
//   e1 = c / |c|, negated if it points against the summed x axes xm = x + R^T x (b to the left of a: images stay upright),
//   e2 = normalize(zm x e1) with zm = z + R^T z the summed optical axes, e3 = e1 x e2.
// Then R_ds_b p_b = R_ds_a p_a - (baseline, 0, 0) with baseline = e1 . c (negative when the sign flipped).
// kRectCoincident: |c| < 1e-9; kRectVertical: the baseline is closer to the images' vertical than to their horizontal,
// |e1 . ym| > |e1 . xm| with ym = y + R^T y.
VC_HD int rectify_rotations(const double* T_ck_a, const double* T_ck_b, double* R_ds_a, double* R_ds_b, double* baseline) {
  double Ra[9], Rb[9], R[9];
  quat_to_R(T_ck_a, Ra); quat_to_R(T_ck_b, Rb);
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) R[3 * i + j] = Rb[3 * i] * Ra[3 * j] + Rb[3 * i + 1] * Ra[3 * j + 1] + Rb[3 * i + 2] * Ra[3 * j + 2];
  double t[3], c[3];
  for (int i = 0; i < 3; ++i) t[i] = T_ck_b[4 + i] - (R[3 * i] * T_ck_a[4] + R[3 * i + 1] * T_ck_a[5] + R[3 * i + 2] * T_ck_a[6]);
  for (int i = 0; i < 3; ++i) c[i] = -(R[i] * t[0] + R[3 + i] * t[1] + R[6 + i] * t[2]);
  const double nc = sqrt(c[0] * c[0] + c[1] * c[1] + c[2] * c[2]);
  if (!(nc >= kRectMinBaseline)) return kRectCoincident;
  double e1[3] = {c[0] / nc, c[1] / nc, c[2] / nc};
  // summed axes in a's frame: column k of I + R^T
  const double xm[3] = {1.0 + R[0], R[1], R[2]}, ym[3] = {R[3], 1.0 + R[4], R[5]}, zm[3] = {R[6], R[7], 1.0 + R[8]};
  const double ex = e1[0] * xm[0] + e1[1] * xm[1] + e1[2] * xm[2], ey = e1[0] * ym[0] + e1[1] * ym[1] + e1[2] * ym[2];
  if (fabs(ey) > fabs(ex)) return kRectVertical;
  if (ex < 0.0) { e1[0] = -e1[0]; e1[1] = -e1[1]; e1[2] = -e1[2]; }
  double e2[3] = {zm[1] * e1[2] - zm[2] * e1[1], zm[2] * e1[0] - zm[0] * e1[2], zm[0] * e1[1] - zm[1] * e1[0]};
  const double n2 = sqrt(e2[0] * e2[0] + e2[1] * e2[1] + e2[2] * e2[2]);
  if (!(n2 > 1e-12)) return kRectVertical;             // the baseline along the mean optical axis: no row geometry either
  e2[0] /= n2; e2[1] /= n2; e2[2] /= n2;
  const double e3[3] = {e1[1] * e2[2] - e1[2] * e2[1], e1[2] * e2[0] - e1[0] * e2[2], e1[0] * e2[1] - e1[1] * e2[0]};
  for (int j = 0; j < 3; ++j) { R_ds_a[j] = e1[j]; R_ds_a[3 + j] = e2[j]; R_ds_a[6 + j] = e3[j]; }
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) R_ds_b[3 * i + j] = R_ds_a[3 * i] * R[3 * j] + R_ds_a[3 * i + 1] * R[3 * j + 1] + R_ds_a[3 * i + 2] * R[3 * j + 2];
  *baseline = e1[0] * c[0] + e1[1] * c[1] + e1[2] * c[2];
  return kRectOk;
}

// W = d(w_a, w_b, baseline) / d(w_ck_a, dp_a, w_ck_b, dp_b), 7 x 12 row-major, in closed form (host): how rectify_rotations' outputs move
// with the two poses.  The poses move as vc_get_solution_covariance's do, q <- q * exp(w_ck) and p <- p + dp; the outputs as
// R_ds <- exp([w]x) R_ds.  With phi = R_ak (w_ck_b - w_ck_a), so that R <- R exp([phi]x), and g = R^T t_bk:
//   dc = -g x phi + dp_a - R^T dp_b,  de1 = (I - e1 e1^T) s dc / |c| (s: the sign flip),  d baseline = e1 . dc,
//   d zm = (R^T z) x phi,  u = zm x e1,  de2 = (I - e2 e2^T)(d zm x e1 + zm x de1) / |u|,  de3 = de1 x e2 + e1 x de2,
//   w_a = (de3 . e2, de1 . e3, de2 . e1),  w_b = w_a - R_ds_a phi.
// The sign flip and the error statuses are rectify_rotations' at the nominal poses, and its status is returned (W untouched on an error).
inline int rect_pose_jacobian(const double* T_ck_a, const double* T_ck_b, double* W) {
  double Rda[9], Rdb[9], b;
  const int rc = rectify_rotations(T_ck_a, T_ck_b, Rda, Rdb, &b);
  if (rc != kRectOk) return rc;
  double Ra[9], Rb[9], R[9];
  quat_to_R(T_ck_a, Ra); quat_to_R(T_ck_b, Rb);
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) R[3 * i + j] = Rb[3 * i] * Ra[3 * j] + Rb[3 * i + 1] * Ra[3 * j + 1] + Rb[3 * i + 2] * Ra[3 * j + 2];
  const double* tb = T_ck_b + 4;
  double g[3];
  for (int i = 0; i < 3; ++i) g[i] = R[i] * tb[0] + R[3 + i] * tb[1] + R[6 + i] * tb[2];
  const double* e1 = Rda; const double* e2 = Rda + 3; const double* e3 = Rda + 6;
  const double nc = std::fabs(b);                                   // |c|: the baseline is s |c|
  const double s = b < 0.0 ? -1.0 : 1.0;
  const double zb[3] = {R[6], R[7], R[8]}, zm[3] = {R[6], R[7], 1.0 + R[8]};
  const double u[3] = {zm[1] * e1[2] - zm[2] * e1[1], zm[2] * e1[0] - zm[0] * e1[2], zm[0] * e1[1] - zm[1] * e1[0]};
  const double n2 = std::sqrt(u[0] * u[0] + u[1] * u[1] + u[2] * u[2]);
  auto cross = [](const double* x, const double* y, double* o) { o[0] = x[1] * y[2] - x[2] * y[1]; o[1] = x[2] * y[0] - x[0] * y[2]; o[2] = x[0] * y[1] - x[1] * y[0]; };
  auto dot = [](const double* x, const double* y) { return x[0] * y[0] + x[1] * y[1] + x[2] * y[2]; };
  for (int col = 0; col < 12; ++col) {
    double d[12] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    d[col] = 1.0;
    const double dw[3] = {d[6] - d[0], d[7] - d[1], d[8] - d[2]};
    double phi[3], dc[3], gxp[3];
    for (int i = 0; i < 3; ++i) phi[i] = Ra[3 * i] * dw[0] + Ra[3 * i + 1] * dw[1] + Ra[3 * i + 2] * dw[2];
    cross(g, phi, gxp);
    for (int i = 0; i < 3; ++i) dc[i] = -gxp[i] + d[3 + i] - (R[i] * d[9] + R[3 + i] * d[10] + R[6 + i] * d[11]);
    const double along = dot(e1, dc);
    double de1[3], dzm[3], t0[3], t1[3], du[3], de2[3], de3[3];
    for (int i = 0; i < 3; ++i) de1[i] = s * (dc[i] - e1[i] * along) / nc;
    cross(zb, phi, dzm);
    cross(dzm, e1, t0); cross(zm, de1, t1);
    for (int i = 0; i < 3; ++i) du[i] = t0[i] + t1[i];
    const double a2 = dot(e2, du);
    for (int i = 0; i < 3; ++i) de2[i] = (du[i] - e2[i] * a2) / n2;
    cross(de1, e2, t0); cross(e1, de2, t1);
    for (int i = 0; i < 3; ++i) de3[i] = t0[i] + t1[i];
    const double wa[3] = {dot(de3, e2), dot(de1, e3), dot(de2, e1)};
    for (int i = 0; i < 3; ++i) {
      W[i * 12 + col] = wa[i];
      W[(3 + i) * 12 + col] = wa[i] - (Rda[3 * i] * phi[0] + Rda[3 * i + 1] * phi[1] + Rda[3 * i + 2] * phi[2]);
    }
    W[6 * 12 + col] = along;
  }
  return kRectOk;
}

// One matched pair of distorted pixels of the same target point.  out = dv = va - vb, d = ua - ub, P = the point in the rectified frame
// of a (Z = fu b / d, X from ua, Y from the mean row), v = (va + vb) / 2.  false (out untouched): an inversion fails (undist_point) or the
// disparity does not have the baseline's sign (d b <= 0: a point behind the pair, or sides swapped).
VC_HD bool rectify_pair(const RectPlan& r, double au, double av, double bu, double bv, double* out) {
  double ua, va, ub, vb;
  if (!undist_point(r.a, au, av, &ua, &va)) return false;
  if (!undist_point(r.b, bu, bv, &ub, &vb)) return false;
  const double d = ua - ub;
  if (!(d * r.baseline > 0.0)) return false;
  const double* dl = r.a.dl;
  const double Z = dl[0] * r.baseline / d, vm = 0.5 * (va + vb);
  out[0] = va - vb; out[1] = d;
  out[2] = (ua - dl[2]) * Z / dl[0]; out[3] = (vm - dl[3]) * Z / dl[1]; out[4] = Z;
  out[5] = vm;
  return true;
}

// ---- rigid fit: the rotation that takes the centred P onto the centred X in the least-squares sense, from H = sum (P - Pm)(X - Xm)^T
// (row-major 3 x 3).  Horn 1987: the unit quaternion is the eigenvector of the largest eigenvalue of the symmetric 4 x 4 matrix N(H).
// One Jacobi rotation of the pair (P, Q), indices known at compile time: everything stays in registers.
template <int P, int Q>
VC_HD void rect_jacobi_rotate(double (&A)[4][4], double (&V)[4][4]) {
  const double apq = A[P][Q];
  const double theta = (A[Q][Q] - A[P][P]) / (2.0 * apq);
  const double tt = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
  const double t = (apq != 0.0 && tt == tt) ? tt : 0.0;       // a zero (or vanishing) off-diagonal element: no rotation
  const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
#pragma unroll
  for (int k = 0; k < 4; ++k) {                                // A <- A J (columns P and Q)
    const double akp = A[k][P], akq = A[k][Q];
    A[k][P] = c * akp - s * akq; A[k][Q] = s * akp + c * akq;
  }
#pragma unroll
  for (int k = 0; k < 4; ++k) {                                // A <- J^T A (rows P and Q)
    const double apk = A[P][k], aqk = A[Q][k];
    A[P][k] = c * apk - s * aqk; A[Q][k] = s * apk + c * aqk;
  }
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const double vkp = V[k][P], vkq = V[k][Q];
    V[k][P] = c * vkp - s * vkq; V[k][Q] = s * vkp + c * vkq;
  }
}
VC_HD void rigid_rotation(const double* H, double* R) {
  const double Sxx = H[0], Sxy = H[1], Sxz = H[2], Syx = H[3], Syy = H[4], Syz = H[5], Szx = H[6], Szy = H[7], Szz = H[8];
  double A[4][4] = {{Sxx + Syy + Szz, Syz - Szy, Szx - Sxz, Sxy - Syx},
                    {Syz - Szy, Sxx - Syy - Szz, Sxy + Syx, Szx + Sxz},
                    {Szx - Sxz, Sxy + Syx, -Sxx + Syy - Szz, Syz + Szy},
                    {Sxy - Syx, Szx + Sxz, Syz + Szy, -Sxx - Syy + Szz}};
  double V[4][4] = {{1, 0, 0, 0}, {0, 1, 0, 0}, {0, 0, 1, 0}, {0, 0, 0, 1}};
  // a fixed number of cyclic sweeps; the sweep's six rotations are written out with constant indices (a rolled loop over the pairs would
  // index the matrices at run time and send them to scratch on the device)
  for (int sweep = 0; sweep < kRectJacobiSweeps; ++sweep) {
    rect_jacobi_rotate<0, 1>(A, V); rect_jacobi_rotate<0, 2>(A, V); rect_jacobi_rotate<0, 3>(A, V);
    rect_jacobi_rotate<1, 2>(A, V); rect_jacobi_rotate<1, 3>(A, V); rect_jacobi_rotate<2, 3>(A, V);
  }
  // the eigenvector of the largest eigenvalue, by selects (the lowest index on ties)
  double best = A[0][0], q0 = V[0][0], q1 = V[1][0], q2 = V[2][0], q3 = V[3][0];
#pragma unroll
  for (int k = 1; k < 4; ++k) {
    const bool up = A[k][k] > best;
    best = up ? A[k][k] : best;
    q0 = up ? V[0][k] : q0; q1 = up ? V[1][k] : q1; q2 = up ? V[2][k] : q2; q3 = up ? V[3][k] : q3;
  }
  const double in = 1.0 / sqrt(q0 * q0 + q1 * q1 + q2 * q2 + q3 * q3);
  const double q[4] = {q1 * in, q2 * in, q3 * in, q0 * in};       // Horn's (w, x, y, z) -> [x y z w]
  quat_to_R(q, R);
}
// |R (P - Pm) - (X - Xm)|^2 of one pair, evaluated explicitly (the expansion sum |P|^2 + sum |X|^2 - 2 tr(R H) cancels to 1e-8 m on exact data)
VC_HD double rigid_residual_sq(const double* R, const double* P, const double* Pm, const double* X, const double* Xm) {
  const double p0 = P[0] - Pm[0], p1 = P[1] - Pm[1], p2 = P[2] - Pm[2];
  const double e0 = R[0] * p0 + R[1] * p1 + R[2] * p2 - (X[0] - Xm[0]);
  const double e1 = R[3] * p0 + R[4] * p1 + R[5] * p2 - (X[1] - Xm[1]);
  const double e2 = R[6] * p0 + R[7] * p1 + R[8] * p2 - (X[2] - Xm[2]);
  return e0 * e0 + e1 * e1 + e2 * e2;
}

}  // namespace vc
