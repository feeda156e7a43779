// vc_seed.hpp -- the arithmetic of the batched planar PnP (vc_seed.hip: vc_pnp_planar_batch), shared with the host build of
// tests/host_harness/seed_harness.cpp.  It restates pnp_planar / pnp_planar_ransac (vc_pnp.hpp) for a group of lanes that hold one
// view together: the lanes stride over the view's corners, every sum over the corners is an all-lane sum of the policy W, and everything
// decided after a sum is the same in all lanes.  W is the wavefront on the device (64 lanes, xor butterfly; vc_seed.hip) and SeedSerial
// on the host (one lane: the strided loops are the plain loops, the sums are the identity).
//   pick sequence   splitmix64 from 0x9E3779B97F4A7C15 ^ n, next() % n, a repeated pick redrawn; the draws run on through the iterations
//   minimal sample  four correspondences fix H exactly: the projective-basis construction (cross products only, no pivoting, no array
//                   indexed at run time) stands in for the host's normalised DLT + Jacobi of the same four points
//   fit             normalised DLT over the used corners (5 + 2 + 45 sums), the 9 x 9 Jacobi eigen-solve with one row of the matrix per
//                   lane (seed_eig9), pose from H (polar iteration, plane offset z0, quaternion), then the host's LM:
//                   lambda 1e-3, damping lambda (H_kk + 1e-12), accept on a smaller cost, x 0.3 (floor 1e-12) / x 10 (give up above
//                   1e12), stop after an accepted step of relative decrease < 1e-12, 50 iterations, 1e6 per corner at depth <= 1e-9 or
//                   with a non-finite residual
//   consensus       error <= tol; more inliers win, on equal count the smaller error sum; < 4: no consensus; refit on the best set,
//                   one re-vote at the refined pose, a second refit only if the re-vote's count is >= 4 and differs
// The unprojection is undist_unproject (analytic slope) instead of the host's numeric-slope Newton: it moves the start of the refinement only.
#pragma once
#include "vc_math.hpp"
#include "vc_undistort.hpp"

// loops over the accumulators are unrolled on the device: every index is a compile-time constant there and the arrays stay in registers
#if defined(__HIPCC__)
#define VC_SEED_UNROLL _Pragma("unroll")
#else
#define VC_SEED_UNROLL
#endif

namespace vc {

enum SeedStatus { kSeedOk = 0, kSeedFewCorners = 1, kSeedNotPlanar = 2, kSeedNoPose = 3, kSeedNoConsensus = 4 };
constexpr int kSeedAcc = 28;                      // 21 (upper triangle of J^T J, row by row) + 6 (J^T r) + 1 (cost)

// ---- the pick sequence of the robust branch ------------------------------------------------------------------------------------
struct SeedSampler { unsigned long long state; };
VC_HD void seed_sampler_init(SeedSampler* s, int n) { s->state = 0x9E3779B97F4A7C15ull ^ (unsigned long long)n; }
VC_HD unsigned long long seed_sampler_next(SeedSampler* s) {
  s->state += 0x9E3779B97F4A7C15ull;
  unsigned long long z = s->state;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}
// four distinct corners of n >= 4 (a repeated pick is drawn again)
VC_HD void seed_pick4(SeedSampler* s, int n, int* p0, int* p1, int* p2, int* p3) {
  const int a = (int)(seed_sampler_next(s) % (unsigned long long)n);
  int b, c, d;
  do { b = (int)(seed_sampler_next(s) % (unsigned long long)n); } while (b == a);
  do { c = (int)(seed_sampler_next(s) % (unsigned long long)n); } while (c == a || c == b);
  do { d = (int)(seed_sampler_next(s) % (unsigned long long)n); } while (d == a || d == b || d == c);
  *p0 = a; *p1 = b; *p2 = c; *p3 = d;
}

// ---- one view ------------------------------------------------------------------------------------------------------------------
struct SeedView {
  int model, n;
  double K[10];
  ModelPre pre;
  const double* pw;      // n x 3
  const double* uv;      // n x 2
  double* xy;            // n x 2 work: the ideal pinhole coordinates of the corners (NaN: no ray), written and read by the same lane
  double z0;
};

VC_HD bool seed_finite(double x) { return fabs(x) <= 1e300; }      // (a NaN fails the comparison)

// pixel -> (x / z, y / z); false beyond the model's field of view (the host's bound: tan > 1e3)
VC_HD bool seed_unproject(const SeedView& s, double u, double v, double* xy) {
  double ray[3];
  if (!undist_unproject(s.model, s.K, s.pre, u, v, ray)) return false;
  if (!(ray[2] > 0.0)) return false;
  const double x = ray[0] / ray[2], y = ray[1] / ray[2];
  if (!(x * x + y * y <= 1e6)) return false;
  xy[0] = x; xy[1] = y;
  return true;
}

VC_HD void seed_cross(const double* a, const double* b, double* o) {
  o[0] = a[1] * b[2] - a[2] * b[1]; o[1] = a[2] * b[0] - a[0] * b[2]; o[2] = a[0] * b[1] - a[1] * b[0];
}
VC_HD double seed_dot(const double* a, const double* b) { return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]; }

// the columns l_k p_k of the map that takes the canonical projective basis to p1 .. p4 (l = adj([p1 p2 p3]) p4: no division)
VC_HD void seed_basis(const double* p1, const double* p2, const double* p3, const double* p4, double* c1, double* c2, double* c3) {
  double x23[3], x31[3], x12[3];
  seed_cross(p2, p3, x23); seed_cross(p3, p1, x31); seed_cross(p1, p2, x12);
  const double l1 = seed_dot(x23, p4), l2 = seed_dot(x31, p4), l3 = seed_dot(x12, p4);
  for (int k = 0; k < 3; ++k) { c1[k] = l1 * p1[k]; c2[k] = l2 * p2[k]; c3[k] = l3 * p3[k]; }
}
// H (row-major, up to scale) with (x, y, 1) ~ H (X, Y, 1) for four correspondences in general position: H = B adj(A)
VC_HD void seed_homography4(const double* X, const double* Y, const double* x, const double* y, double* H) {
  double P[4][3], Q[4][3];
  for (int k = 0; k < 4; ++k) { P[k][0] = X[k]; P[k][1] = Y[k]; P[k][2] = 1.0; Q[k][0] = x[k]; Q[k][1] = y[k]; Q[k][2] = 1.0; }
  double a1[3], a2[3], a3[3], b1[3], b2[3], b3[3], r1[3], r2[3], r3[3];
  seed_basis(P[0], P[1], P[2], P[3], a1, a2, a3);
  seed_basis(Q[0], Q[1], Q[2], Q[3], b1, b2, b3);
  seed_cross(a2, a3, r1); seed_cross(a3, a1, r2); seed_cross(a1, a2, r3);      // the rows of adj(A)
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) H[3 * i + j] = b1[i] * r1[j] + b2[i] * r2[j] + b3[i] * r3[j];
}

// T_cw = [q (x y z w) | t] from H = lambda [r1 r2 t'] of the plane z = z0 (t = t' - r3 z0), as pnp_planar_masked does it
VC_HD bool seed_pose_from_H(const double* H, double z0, double* T) {
  double r1[3] = {H[0], H[3], H[6]}, r2[3] = {H[1], H[4], H[7]}, t[3] = {H[2], H[5], H[8]};
  const double n1 = sqrt(seed_dot(r1, r1)), n2 = sqrt(seed_dot(r2, r2));
  if (!(n1 > 0) || !(n2 > 0)) return false;
  double lam = 2.0 / (n1 + n2);
  if (t[2] * lam < 0) lam = -lam;                 // the target is in front of the camera
  for (int i = 0; i < 3; ++i) { r1[i] *= lam; r2[i] *= lam; t[i] *= lam; }
  double r3[3], R[9];
  seed_cross(r1, r2, r3);
  for (int i = 0; i < 3; ++i) { R[3 * i] = r1[i]; R[3 * i + 1] = r2[i]; R[3 * i + 2] = r3[i]; }
  for (int it = 0; it < 30; ++it) {               // nearest rotation: Newton polar iteration R <- (R + R^-T) / 2
    const double c00 = R[4] * R[8] - R[5] * R[7], c01 = R[5] * R[6] - R[3] * R[8], c02 = R[3] * R[7] - R[4] * R[6];
    const double det = R[0] * c00 + R[1] * c01 + R[2] * c02;
    if (!(fabs(det) >= 1e-12)) return false;
    const double cof[9] = {c00, c01, c02,
                           R[2] * R[7] - R[1] * R[8], R[0] * R[8] - R[2] * R[6], R[1] * R[6] - R[0] * R[7],
                           R[1] * R[5] - R[2] * R[4], R[2] * R[3] - R[0] * R[5], R[0] * R[4] - R[1] * R[3]};
    double diff = 0;
    for (int k = 0; k < 9; ++k) { const double nr = 0.5 * (R[k] + cof[k] / det); diff += fabs(nr - R[k]); R[k] = nr; }
    if (diff < 1e-15) break;
  }
  for (int i = 0; i < 3; ++i) t[i] -= R[3 * i + 2] * z0;
  double q[4];
  const double tr = R[0] + R[4] + R[8];
  if (tr > 0) { const double s = sqrt(tr + 1.0) * 2; q[3] = 0.25 * s; q[0] = (R[7] - R[5]) / s; q[1] = (R[2] - R[6]) / s; q[2] = (R[3] - R[1]) / s; }
  else if (R[0] > R[4] && R[0] > R[8]) { const double s = sqrt(1.0 + R[0] - R[4] - R[8]) * 2; q[3] = (R[7] - R[5]) / s; q[0] = 0.25 * s; q[1] = (R[1] + R[3]) / s; q[2] = (R[2] + R[6]) / s; }
  else if (R[4] > R[8]) { const double s = sqrt(1.0 + R[4] - R[0] - R[8]) * 2; q[3] = (R[2] - R[6]) / s; q[0] = (R[1] + R[3]) / s; q[1] = 0.25 * s; q[2] = (R[5] + R[7]) / s; }
  else { const double s = sqrt(1.0 + R[8] - R[0] - R[4]) * 2; q[3] = (R[3] - R[1]) / s; q[0] = (R[2] + R[6]) / s; q[1] = (R[5] + R[7]) / s; q[2] = 0.25 * s; }
  const double nq = sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
  for (int i = 0; i < 4; ++i) T[i] = q[i] / nq;
  for (int i = 0; i < 3; ++i) T[4 + i] = t[i];
  return seed_finite(t[0] + t[1] + t[2]);
}

// the rough pose of one minimal sample (one lane; nothing here is shared with another lane)
VC_HD bool seed_minimal_pose(const SeedView& s, int p0, int p1, int p2, int p3, double* T) {
  const int pick[4] = {p0, p1, p2, p3};
  double X[4], Y[4], x[4], y[4];
  bool ok = true;
  for (int k = 0; k < 4; ++k) {
    const size_t i = (size_t)pick[k];
    double xy[2] = {0.0, 0.0};
    ok = seed_unproject(s, s.uv[2 * i], s.uv[2 * i + 1], xy) && ok;
    X[k] = s.pw[3 * i]; Y[k] = s.pw[3 * i + 1]; x[k] = xy[0]; y[k] = xy[1];
  }
  if (!ok) return false;
  double H[9];
  seed_homography4(X, Y, x, y, H);
  return seed_pose_from_H(H, s.z0, T);
}

// ---- the 9 x 9 symmetric eigen-solve: cyclic Jacobi (jacobi_eig of vc_pnp.hpp) with the rows of A and of V held by their OWNERS --------
// Owner k has row k of A and row k of V.  On the device lane k owns row k (lanes 9 .. 63 own a row of zeros): 18 doubles in registers, every
// index a compile-time constant of the unrolled (p, q) loops, no LDS, no array indexed at run time.  One lane of the host build owns all nine.
// A rotation (p, q): c and s from A_pp, A_qq, A_pq (lane reads: the same in every lane); every owner rotates columns p and q of its rows of A
// and V; the owners of rows p and q then replace them by the rotated pair.  The same operations in the same order as the serial routine.
VC_HD bool seed_rot_coeffs(double app, double aqq, double apq, double* c, double* s) {
  if (fabs(apq) < 1e-300) return false;
  const double theta = (aqq - app) / (2.0 * apq);
  const double t = (theta >= 0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
  *c = 1.0 / sqrt(t * t + 1.0); *s = t * *c;
  return true;
}
// entry `col` of the row that owner `row` holds (m: this lane's rows), in every lane
template <int NO, class W>
VC_HD double seed_owner_value(const W& w, const double (*m)[9], int row, int col) {
  if constexpr (NO == 9) return m[row][col];
  else return w.bcast(m[0][col], row);
}
// acc: the packed upper triangle of A (45, row by row), the same in every lane.  Hn: the eigenvector of the smallest eigenvalue, in every lane.
template <class W>
VC_HD void seed_eig9(const W& w, const double* acc, double* Hn) {
  constexpr int NO = W::kLanes == 1 ? 9 : 1;      // rows one lane owns
  double a[NO][9], v[NO][9];
  VC_SEED_UNROLL
  for (int o = 0; o < NO; ++o) {
    const int k = NO == 9 ? o : w.lane;
    VC_SEED_UNROLL
    for (int j = 0; j < 9; ++j) {
      double x = 0.0;
      VC_SEED_UNROLL
      for (int r = 0; r < 9; ++r) {
        const int lo = r < j ? r : j, hi = r < j ? j : r;
        if (k == r) x = acc[lo * 9 - (lo * (lo - 1)) / 2 + (hi - lo)];
      }
      a[o][j] = x; v[o][j] = k == j ? 1.0 : 0.0;
    }
  }
  for (int sweep = 0; sweep < 60; ++sweep) {
    double off = 0.0;
    VC_SEED_UNROLL
    for (int o = 0; o < NO; ++o) {
      const int k = NO == 9 ? o : w.lane;
      VC_SEED_UNROLL
      for (int j = 1; j < 9; ++j) if (j > k) off += a[o][j] * a[o][j];
    }
    off = w.allsum(off);
    if (off < 1e-300) break;
    VC_SEED_UNROLL
    for (int p = 0; p < 9; ++p) {
      VC_SEED_UNROLL
      for (int q = p + 1; q < 9; ++q) {
        double c, s;
        if (!seed_rot_coeffs(seed_owner_value<NO>(w, a, p, p), seed_owner_value<NO>(w, a, q, q), seed_owner_value<NO>(w, a, p, q), &c, &s)) continue;
        VC_SEED_UNROLL
        for (int o = 0; o < NO; ++o) {
          const double ap = a[o][p], aq = a[o][q], vp = v[o][p], vq = v[o][q];
          a[o][p] = c * ap - s * aq; a[o][q] = s * ap + c * aq;
          v[o][p] = c * vp - s * vq; v[o][q] = s * vp + c * vq;
        }
        double rp[9], rq[9];
        VC_SEED_UNROLL
        for (int j = 0; j < 9; ++j) { rp[j] = seed_owner_value<NO>(w, a, p, j); rq[j] = seed_owner_value<NO>(w, a, q, j); }
        VC_SEED_UNROLL
        for (int o = 0; o < NO; ++o) {
          const int k = NO == 9 ? o : w.lane;
          VC_SEED_UNROLL
          for (int j = 0; j < 9; ++j) {
            if (k == p) a[o][j] = c * rp[j] - s * rq[j];
            else if (k == q) a[o][j] = s * rp[j] + c * rq[j];
          }
        }
      }
    }
  }
  int best = 0;
  double dbest = seed_owner_value<NO>(w, a, 0, 0);
  VC_SEED_UNROLL
  for (int k = 1; k < 9; ++k) {
    const double d = seed_owner_value<NO>(w, a, k, k);
    if (d < dbest) { dbest = d; best = k; }
  }
  double vb[NO][9];                                // ([o][0]: column `best` of the owner's rows of V)
  VC_SEED_UNROLL
  for (int o = 0; o < NO; ++o) {
    double x = v[o][0];
    VC_SEED_UNROLL
    for (int j = 1; j < 9; ++j) if (best == j) x = v[o][j];
    vb[o][0] = x;
  }
  VC_SEED_UNROLL
  for (int k = 0; k < 9; ++k) Hn[k] = seed_owner_value<NO>(w, vb, k, 0);
}

VC_HD bool seed_used(const char* use, size_t i) { return !use || use[i]; }

// H (row-major, up to scale) of the used points by the normalised DLT  s [x y 1]^T = H [X Y 1]^T: Hartley normalisation (5 + 2 sums), the 45 sums
// of the upper triangle of A^T A, seed_eig9, de-normalisation.  pt(i, &X, &Y, &x, &y) gives point i of n and whether it is used; every lane gets
// the same H.  *m_used (nullable) gets the number of used points.  false: fewer than 4 used points, or all of them on one spot.
template <class W, class P>
VC_HD bool seed_dlt_H(const W& w, int n, const P& pt, double* H, int* m_used = nullptr) {
  int m = 0;
  double mX = 0, mY = 0, mx = 0, my = 0;
  for (int i = w.lane; i < n; i += W::kLanes) {
    double X, Y, x, y;
    if (pt(i, &X, &Y, &x, &y)) { ++m; mX += X; mY += Y; mx += x; my += y; }
  }
  m = w.allsum(m);
  if (m_used) *m_used = m;
  if (m < 4) return false;
  mX = w.allsum(mX) / m; mY = w.allsum(mY) / m; mx = w.allsum(mx) / m; my = w.allsum(my) / m;
  double dW = 0, dI = 0;
  for (int i = w.lane; i < n; i += W::kLanes) {
    double X, Y, x, y;
    if (pt(i, &X, &Y, &x, &y)) {
      const double a = X - mX, b = Y - mY, c = x - mx, d = y - my;
      dW += sqrt(a * a + b * b); dI += sqrt(c * c + d * d);
    }
  }
  dW = w.allsum(dW); dI = w.allsum(dI);
  if (!(dW > 0) || !(dI > 0)) return false;
  const double sW = sqrt(2.0) * m / dW, sI = sqrt(2.0) * m / dI;
  double acc[45];
  VC_SEED_UNROLL
  for (int k = 0; k < 45; ++k) acc[k] = 0.0;
  for (int i = w.lane; i < n; i += W::kLanes) {
    double Xi, Yi, xi, yi;
    if (!pt(i, &Xi, &Yi, &xi, &yi)) continue;
    const double X = (Xi - mX) * sW, Y = (Yi - mY) * sW, x = (xi - mx) * sI, y = (yi - my) * sI;
    const double r1[9] = {-X, -Y, -1, 0, 0, 0, x * X, x * Y, x}, r2[9] = {0, 0, 0, -X, -Y, -1, y * X, y * Y, y};
    int k = 0;
  VC_SEED_UNROLL
    for (int a = 0; a < 9; ++a)
  VC_SEED_UNROLL
      for (int b = a; b < 9; ++b) acc[k++] += r1[a] * r1[b] + r2[a] * r2[b];
  }
  VC_SEED_UNROLL
  for (int k = 0; k < 45; ++k) acc[k] = w.allsum(acc[k]);
  double Hn[9];
  seed_eig9(w, acc, Hn);                          // the eigenvector of the smallest eigenvalue
  // de-normalise: H = Ti^-1 Hn Tw with Tw = [sW 0 -sW mX; 0 sW -sW mY; 0 0 1], Ti likewise
  const double Tw[9] = {sW, 0, -sW * mX, 0, sW, -sW * mY, 0, 0, 1}, TiInv[9] = {1 / sI, 0, mx, 0, 1 / sI, my, 0, 0, 1};
  double tmp[9];
  for (int i = 0; i < 3; ++i) for (int j = 0; j < 3; ++j) { tmp[3 * i + j] = 0; for (int k = 0; k < 3; ++k) tmp[3 * i + j] += Hn[3 * i + k] * Tw[3 * k + j]; }
  for (int i = 0; i < 3; ++i) for (int j = 0; j < 3; ++j) { H[3 * i + j] = 0; for (int k = 0; k < 3; ++k) H[3 * i + j] += TiInv[3 * i + k] * tmp[3 * k + j]; }
  return true;
}

// the used corners of a view for seed_dlt_H: target (X, Y) against the ideal pinhole coordinates kept in s.xy
struct SeedPosePoints {
  const SeedView& s;
  const char* use;
  VC_HD bool operator()(int i, double* X, double* Y, double* x, double* y) const {
    *x = s.xy[2 * (size_t)i]; *y = s.xy[2 * (size_t)i + 1];
    *X = s.pw[3 * (size_t)i]; *Y = s.pw[3 * (size_t)i + 1];
    return seed_used(use, i) && *x == *x;
  }
};

// rough pose of the used corners: seed_dlt_H, then seed_pose_from_H
template <class W>
VC_HD bool seed_dlt_pose(const W& w, const SeedView& s, const char* use, double* T) {
  double H[9];
  if (!seed_dlt_H(w, s.n, SeedPosePoints{s, use}, H)) return false;
  return seed_pose_from_H(H, s.z0, T);
}

// corner i in the camera frame of the pose (Rc, tc)
VC_HD void seed_point(const SeedView& s, const double* Rc, const double* Tc, size_t i, double* p, double* pc) {
  p[0] = s.pw[3 * i]; p[1] = s.pw[3 * i + 1]; p[2] = s.pw[3 * i + 2];
  for (int a = 0; a < 3; ++a) pc[a] = Rc[3 * a] * p[0] + Rc[3 * a + 1] * p[1] + Rc[3 * a + 2] * p[2] + Tc[4 + a];
}

// One sweep of the refinement over the used corners at pose Tc, summed over the lanes: the cost, the number of corners it went over
// and, with JAC, Hu (21, the upper triangle of J^T J) and g (6, J^T r) of T_cw <- T_cw exp(delta).
template <bool JAC, class W>
VC_HD double seed_cost(const W& w, const SeedView& s, const char* use, const double* Tc, double* Hu, double* g, int* n_cost) {
  double Rc[9];
  quat_to_R(Tc, Rc);
  double acc[kSeedAcc];
  VC_SEED_UNROLL
  for (int k = 0; k < kSeedAcc; ++k) acc[k] = 0.0;
  int cnt = 0;
  for (int i = w.lane; i < s.n; i += W::kLanes) {
    if (!seed_used(use, i)) continue;
    ++cnt;
    double p[3], pc[3], pix[2], A[6], B[20];
    seed_point(s, Rc, Tc, (size_t)i, p, pc);
    if (pc[2] <= 1e-9) { acc[27] += 1e6; continue; }
    project_any<JAC>(s.model, pc, s.K, s.pre, pix, JAC ? A : nullptr, JAC ? B : nullptr);
    const double r0 = pix[0] - s.uv[2 * (size_t)i], r1 = pix[1] - s.uv[2 * (size_t)i + 1];
    if (!seed_finite(r0) || !seed_finite(r1)) { acc[27] += 1e6; continue; }
    acc[27] += r0 * r0 + r1 * r1;
    if (JAC) {
      // d pc / d upsilon = R,  d pc / d omega = -R [p]x
      double J[12];
  VC_SEED_UNROLL
      for (int a = 0; a < 2; ++a) {
        double AR[3];
        for (int b = 0; b < 3; ++b) AR[b] = A[3 * a] * Rc[b] + A[3 * a + 1] * Rc[3 + b] + A[3 * a + 2] * Rc[6 + b];
        J[6 * a] = AR[0]; J[6 * a + 1] = AR[1]; J[6 * a + 2] = AR[2];
        J[6 * a + 3] = -(AR[1] * p[2] - AR[2] * p[1]);
        J[6 * a + 4] = -(AR[2] * p[0] - AR[0] * p[2]);
        J[6 * a + 5] = -(AR[0] * p[1] - AR[1] * p[0]);
      }
      int k = 0;
  VC_SEED_UNROLL
      for (int a = 0; a < 6; ++a) {
  VC_SEED_UNROLL
        for (int b = a; b < 6; ++b) acc[k++] += J[a] * J[b] + J[6 + a] * J[6 + b];
        acc[21 + a] += J[a] * r0 + J[6 + a] * r1;
      }
    }
  }
  if (JAC) {
  VC_SEED_UNROLL
    for (int k = 0; k < 21; ++k) Hu[k] = w.allsum(acc[k]);
  VC_SEED_UNROLL
    for (int k = 0; k < 6; ++k) g[k] = w.allsum(acc[21 + k]);
  }
  *n_cost = w.allsum(cnt);
  return w.allsum(acc[27]);
}

// LM refinement of T over the used corners; *rms = sqrt(cost / corners used) at the returned pose
template <class W>
VC_HD bool seed_refine(const W& w, const SeedView& s, const char* use, double* T, double* rms) {
  double lambda = 1e-3, Hu[21], g[6];
  int n_cost = 0, n_trial = 0;
  double cost = seed_cost<true>(w, s, use, T, Hu, g, &n_cost);
  for (int it = 0; it < 50; ++it) {
    double M[36], d[6];
    {
      int k = 0;
  VC_SEED_UNROLL
      for (int a = 0; a < 6; ++a)
  VC_SEED_UNROLL
        for (int b = a; b < 6; ++b) { M[a * 6 + b] = Hu[k]; M[b * 6 + a] = Hu[k]; ++k; }
    }
  VC_SEED_UNROLL
    for (int k = 0; k < 6; ++k) { M[7 * k] += lambda * (M[7 * k] + 1e-12); d[k] = -g[k]; }
    if (!chol_small<6>(M)) { lambda *= 10; if (lambda > 1e12) break; continue; }
    fwd_solve<6>(M, d); bwd_solve<6>(M, d);
    double Tn[7];
    se3_plus(T, d, Tn);
    const double cn = seed_cost<false>(w, s, use, Tn, nullptr, nullptr, &n_trial);
    if (cn < cost) {
      const double rel = (cost - cn) / (cost + 1e-300);
      for (int k = 0; k < 7; ++k) T[k] = Tn[k];
      cost = seed_cost<true>(w, s, use, T, Hu, g, &n_cost);
      lambda = fmax(lambda * 0.3, 1e-12);
      if (rel < 1e-12) break;
    } else { lambda *= 10; if (lambda > 1e12) break; }
  }
  *rms = sqrt(cost / (n_cost > 0 ? n_cost : 1));
  return seed_finite(cost);
}

// the vote of every corner at pose T: count and error sum of the corners within tol; mask (nullable) gets the flags
template <class W>
VC_HD void seed_vote(const W& w, const SeedView& s, const double* T, double tol, char* mask, int* count, double* sum) {
  double Rc[9];
  quat_to_R(T, Rc);
  int cnt = 0;
  double sm = 0.0;
  for (int i = w.lane; i < s.n; i += W::kLanes) {
    double p[3], pc[3], pix[2], e = 1e30;
    seed_point(s, Rc, T, (size_t)i, p, pc);
    if (!(pc[2] <= 1e-9)) {
      project_any<false>(s.model, pc, s.K, s.pre, pix, nullptr, nullptr);
      const double a = pix[0] - s.uv[2 * (size_t)i], b = pix[1] - s.uv[2 * (size_t)i + 1];
      e = sqrt(a * a + b * b);
      if (!seed_finite(e)) e = 1e30;
    }
    const bool in = e <= tol;
    if (in) { ++cnt; sm += e; }
    if (mask) mask[i] = in ? 1 : 0;
  }
  *count = w.allsum(cnt);
  *sum = w.allsum(sm);
}

// The whole view.  mask: 2 n flags of work (written and read by the same lane).  Returns the status; with kSeedOk T (7), *rms, *n_inliers and
// *inlier (the flags of the returned set inside mask, or nullptr: every corner) are set, the same in every lane.
template <class W>
VC_HD int seed_view(const W& w, SeedView& s, int its, double tol, char* mask, double* T, double* rms, int* n_inliers, const char** inlier) {
  const int n = s.n;
  if (n < 4) return kSeedFewCorners;
  s.z0 = s.pw[2];
  int off_plane = 0;
  for (int i = w.lane; i < n; i += W::kLanes) if (fabs(s.pw[3 * (size_t)i + 2] - s.z0) > 1e-9) ++off_plane;
  if (w.allsum(off_plane) > 0) return kSeedNotPlanar;
  const double nan = __builtin_nan("");
  for (int i = w.lane; i < n; i += W::kLanes) {
    double xy[2];
    const bool ok = seed_unproject(s, s.uv[2 * (size_t)i], s.uv[2 * (size_t)i + 1], xy);
    s.xy[2 * (size_t)i] = ok ? xy[0] : nan; s.xy[2 * (size_t)i + 1] = ok ? xy[1] : nan;
  }
  const bool robust = !(its <= 0 || n < 5);
  int best_cnt = 0;
  double Tb[7] = {0, 0, 0, 1, 0, 0, 0};
  if (robust) {
    // ---- lane = hypothesis for the minimal-sample poses, then the lanes walk the hypotheses of the round together ----
    double best_sum = 0.0;
    SeedSampler smp;
    seed_sampler_init(&smp, n);
    for (int left = its; left > 0; left -= W::kLanes) {
      const int round = left < W::kLanes ? left : W::kLanes;
      int p0 = 0, p1 = 0, p2 = 0, p3 = 0;
      for (int j = 0; j < round; ++j) {           // every lane draws the whole sequence: the draws of iteration k depend on those before it
        int q0, q1, q2, q3;
        seed_pick4(&smp, n, &q0, &q1, &q2, &q3);
        if (j == w.lane) { p0 = q0; p1 = q1; p2 = q2; p3 = q3; }
      }
      double Th[7] = {0, 0, 0, 1, 0, 0, 0};
      int hok = 0;
      if (w.lane < round) hok = seed_minimal_pose(s, p0, p1, p2, p3, Th) ? 1 : 0;
      for (int j = 0; j < round; ++j) {
        if (!w.bcast(hok, j)) continue;
        double Tj[7];
        for (int k = 0; k < 7; ++k) Tj[k] = w.bcast(Th[k], j);
        int cnt; double sum;
        seed_vote(w, s, Tj, tol, nullptr, &cnt, &sum);
        if (cnt > best_cnt || (cnt == best_cnt && cnt > 0 && sum < best_sum)) {
          best_cnt = cnt; best_sum = sum;
          for (int k = 0; k < 7; ++k) Tb[k] = Tj[k];
        }
      }
    }
    if (best_cnt < 4) return kSeedNoConsensus;
    int cnt; double sum;
    seed_vote(w, s, Tb, tol, mask, &cnt, &sum);   // the best hypothesis's mask again, from its pose
  }
  // ---- fit on all corners (plain) or on the consensus set; the refined pose re-votes once (a minimal sample's pose is rough) ----
  const char* use = robust ? mask : nullptr;
  int n_use = robust ? best_cnt : n;
  for (int fit = 0; fit < (robust ? 2 : 1); ++fit) {
    const char* cand = use;
    int n_cand = n_use;
    if (fit == 1) {
      double sum;
      seed_vote(w, s, T, tol, mask + n, &n_cand, &sum);
      if (!(n_cand >= 4 && n_cand != n_use)) break;
      cand = mask + n;
    }
    double Tf[7], r = 0.0;
    if (!(seed_dlt_pose(w, s, cand, Tf) && seed_refine(w, s, cand, Tf, &r))) {
      if (fit == 0) return kSeedNoPose;
      break;                                      // (a failed second fit leaves the first)
    }
    for (int k = 0; k < 7; ++k) T[k] = Tf[k];
    *rms = r; use = cand; n_use = n_cand;
  }
  *n_inliers = n_use; *inlier = use;
  return kSeedOk;
}

// one lane holds the whole view: the host build
struct SeedSerial {
  static constexpr int kLanes = 1;
  int lane = 0;
  double allsum(double x) const { return x; }
  int allsum(int x) const { return x; }
  int allmin(int x) const { return x; }
  double bcast(double x, int) const { return x; }
  int bcast(int x, int) const { return x; }
};

// ---- the host side of vc_seed.hip (vc_pnp_planar_batch and the calibrator's device seeding go through it) ------------------------
// stream: a hipStream_t of `device`, or nullptr for the null stream.  The arguments are those of vc_pnp_planar_batch, already checked.
// kernel_ms (nullable): the mean time of the kernel alone over time_reps more launches on the same input, back to back between two events.
int seed_batch_run(int device, void* stream, int n_views, const int* view_model, const double* view_K, const int* view_off, const double* p_w,
                   const double* p_c, int iterations, double tol_px, double* T_cw, double* rms, int* n_inliers, char* inlier, int* status,
                   int time_reps = 0, double* kernel_ms = nullptr);
bool seed_batch_args_ok(int n_views, const int* view_model, const double* view_K, const int* view_off, const double* p_w, const double* p_c,
                        int iterations, double tol_px, const double* T_cw, const double* rms, const int* n_inliers, const int* status);

}  // namespace vc
