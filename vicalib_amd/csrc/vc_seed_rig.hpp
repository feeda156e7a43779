// vc_seed_rig.hpp -- the arithmetic of the rig seed (vc_seed_rig): every camera's pose relative to camera 0 from the frames two cameras
// share.  VC_HD: the kernels of vc_seed_rig.hip and the host harness of the tests (tests/host_harness/seed_rig_harness.cpp) run the very
// same functions; what the kernels add is the order of the sums.  The index of shared frames, the argument checks and the spanning tree
// are plain host C++.
//
// A pose is [qx qy qz qw tx ty tz] with a unit quaternion.  A candidate is 8 doubles: the pose X = T_aw T_bw^-1 (camera b into camera a;
// its quaternion normalised) and the scale d = max(|t_aw|, |t_bw|).
#pragma once
#include <cmath>
#include "vc_math.hpp"
#include <vector>

namespace vc {

constexpr int kSeedRigMaxCams = 8;                     // (= kMaxCams of vc_device.h; vc_seed_rig.hip asserts it)
constexpr int kSeedRigMaxPairs = kSeedRigMaxCams * (kSeedRigMaxCams - 1) / 2;
constexpr int kSeedRigMaxFrames = 1 << 17;             // 28 pairs x 2^17 candidates x 64 B = 235 MB on the device; the vote is quadratic in it
constexpr int kSeedRigTile = 256;                      // candidates per workgroup and per LDS tile of the vote
constexpr int kSeedRigRec = 8;                         // doubles per candidate
enum { kSeedRigOk = 0, kSeedRigNoShared = 1, kSeedRigFewSupport = 2 };
enum { kSeedRigReached = 0, kSeedRigNotConnected = 1 };

VC_HD int srig_n_pairs(int n_cams) { return n_cams * (n_cams - 1) / 2; }
// the place of pair (a < b) in the order (0,1), (0,2) .. (0,C-1), (1,2) ..
VC_HD int srig_pair_index(int n_cams, int a, int b) { return a * (n_cams - 1) - (a * (a - 1)) / 2 + (b - a - 1); }

VC_HD void srig_candidate(const double* Ta, const double* Tb, double* X) {
  const double cb[4] = {-Tb[0], -Tb[1], -Tb[2], Tb[3]};
  double q[4], r[3];
  quat_mul(Ta, cb, q);
  const double in = 1.0 / sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
  q[0] *= in; q[1] *= in; q[2] *= in; q[3] *= in;
  quat_rotate(q, Tb + 4, r);
  X[0] = q[0]; X[1] = q[1]; X[2] = q[2]; X[3] = q[3];
  X[4] = Ta[4] - r[0]; X[5] = Ta[5] - r[1]; X[6] = Ta[6] - r[2];
  const double da = sqrt(Ta[4] * Ta[4] + Ta[5] * Ta[5] + Ta[6] * Ta[6]), db = sqrt(Tb[4] * Tb[4] + Tb[5] * Tb[5] + Tb[6] * Tb[6]);
  X[7] = da > db ? da : db;
}

// the two thresholds of the vote, computed once on the host: cos(tol / 2) and tol^2 (radians)
struct SrigTol { double cos_half, tol2; };
inline SrigTol srig_tol(double tol_deg) {
  const double r = tol_deg * (3.14159265358979323846 / 180.0);
  return SrigTol{std::cos(0.5 * r), r * r};
}

// candidates i and j agree: |q_i . q_j| >= cos(tol / 2) and |t_i - t_j|^2 <= tol^2 (d_i + d_j)^2.  No acos.  Symmetric in i and j.
VC_HD bool srig_agree(const double* Xi, const double* Xj, double cos_half, double tol2) {
  const double dot = Xi[0] * Xj[0] + Xi[1] * Xj[1] + Xi[2] * Xj[2] + Xi[3] * Xj[3];
  const double dx = Xi[4] - Xj[4], dy = Xi[5] - Xj[5], dz = Xi[6] - Xj[6];
  const double s = Xi[7] + Xj[7];
  const bool turn = fabs(dot) >= cos_half, move = dx * dx + dy * dy + dz * dz <= tol2 * (s * s);
  return turn & move;                                                // (both evaluated: no branch between the two in the vote's inner loop)
}

// one agreeing candidate's share of the refit: acc[0..3] += +-q (the winner's hemisphere), acc[4..6] += t
VC_HD void srig_refit_term(const double* W, const double* X, double* acc) {
  const double dot = W[0] * X[0] + W[1] * X[1] + W[2] * X[2] + W[3] * X[3];
  const double s = dot < 0.0 ? -1.0 : 1.0;
  acc[0] += s * X[0]; acc[1] += s * X[1]; acc[2] += s * X[2]; acc[3] += s * X[3];
  acc[4] += X[4]; acc[5] += X[5]; acc[6] += X[6];
}
// q = normalise(sum) with qw >= 0, t = the mean
VC_HD void srig_refit_finish(const double* acc, int count, double* T) {
  double in = 1.0 / sqrt(acc[0] * acc[0] + acc[1] * acc[1] + acc[2] * acc[2] + acc[3] * acc[3]);
  if (acc[3] < 0.0) in = -in;
  T[0] = acc[0] * in; T[1] = acc[1] * in; T[2] = acc[2] * in; T[3] = acc[3] * in;
  const double ic = 1.0 / (double)count;
  T[4] = acc[4] * ic; T[5] = acc[5] * ic; T[6] = acc[6] * ic;
}
// one agreeing candidate's share of the two spreads: the squared angle between T and X, 2 atan2(|vec|, |w|) of T.q^-1 X.q, and |X.t - T.t|^2
VC_HD void srig_spread_term(const double* T, const double* X, double* ang2, double* dist2) {
  const double ct[4] = {-T[0], -T[1], -T[2], T[3]};
  double r[4];
  quat_mul(ct, X, r);
  const double a = 2.0 * atan2(sqrt(r[0] * r[0] + r[1] * r[1] + r[2] * r[2]), fabs(r[3]));
  const double dx = X[4] - T[4], dy = X[5] - T[5], dz = X[6] - T[6];
  *ang2 += a * a;
  *dist2 += dx * dx + dy * dy + dz * dz;
}
VC_HD void srig_spread_finish(double ang2, double dist2, int count, double* rms_deg, double* rms_m) {
  const double ic = 1.0 / (double)count;
  *rms_deg = sqrt(ang2 * ic) * (180.0 / 3.14159265358979323846);
  *rms_m = sqrt(dist2 * ic);
}

// ---- host only ------------------------------------------------------------------------------------------------------------------------
// 0, -2 (VC_ERR_BAD_ARG) or -7 (VC_ERR_UNSUPPORTED); judged before anything is read
inline int srig_judge(int n_frames, int n_cams, const void* view_ok, const void* view_T_cw, double tol_deg, int min_support, bool outputs_ok) {
  if (!view_ok || !view_T_cw || !outputs_ok) return -2;
  if (n_frames < 0 || n_cams < 1 || !(tol_deg > 0.0) || !(tol_deg < 90.0) || min_support < 1) return -2;
  if (n_cams > kSeedRigMaxCams || n_frames > kSeedRigMaxFrames) return -7;
  return 0;
}

// The frames every pair shares, in frame order: pair p owns entries off[p] .. off[p] + n[p] - 1 of `frame`.  Only view_ok is read.
struct SrigIndex {
  int n_pairs = 0;
  int a[kSeedRigMaxPairs], b[kSeedRigMaxPairs], off[kSeedRigMaxPairs], n[kSeedRigMaxPairs];
  int n_max = 0;
  std::vector<int> frame;
};
inline void srig_build_index(int n_frames, int n_cams, const unsigned char* view_ok, SrigIndex* ix) {
  ix->n_pairs = srig_n_pairs(n_cams); ix->n_max = 0; ix->frame.clear();
  int p = 0;
  for (int a = 0; a < n_cams; ++a)
    for (int b = a + 1; b < n_cams; ++b, ++p) {
      ix->a[p] = a; ix->b[p] = b; ix->off[p] = (int)ix->frame.size();
      for (int k = 0; k < n_frames; ++k)
        if (view_ok[(size_t)k * n_cams + a] && view_ok[(size_t)k * n_cams + b]) ix->frame.push_back(k);
      ix->n[p] = (int)ix->frame.size() - ix->off[p];
      if (ix->n[p] > ix->n_max) ix->n_max = ix->n[p];
    }
}

inline void srig_pose_mul(const double* A, const double* B, double* O) {        // O = A B, the quaternion normalised with qw >= 0
  double q[4], r[3];
  quat_mul(A, B, q);
  quat_rotate(A, B + 4, r);
  double in = 1.0 / std::sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
  if (q[3] < 0.0) in = -in;
  O[0] = q[0] * in; O[1] = q[1] * in; O[2] = q[2] * in; O[3] = q[3] * in;
  O[4] = A[4] + r[0]; O[5] = A[5] + r[1]; O[6] = A[6] + r[2];
}
inline void srig_pose_inv(const double* A, double* O) {
  const double c[4] = {-A[0], -A[1], -A[2], A[3]};
  double r[3];
  quat_rotate(c, A + 4, r);
  O[0] = c[0]; O[1] = c[1]; O[2] = c[2]; O[3] = c[3]; O[4] = -r[0]; O[5] = -r[1]; O[6] = -r[2];
}

// The rig: a maximum spanning tree over the status-0 pairs weighted by support, grown from camera 0 by Prim's rule; ties go to the lowest
// tree camera, then to the lowest new camera.  cam_T_c0[c] takes camera 0 into camera c (camera 0: the identity), composed along the
// tree; cam_parent is -1 for camera 0 and for a camera not reached, whose pose is left as it was.
inline void srig_tree(int n_cams, const int* pair_status, const int* pair_support, const double* pair_T_ab, double* cam_T_c0, int* cam_parent, int* cam_status) {
  bool in_tree[kSeedRigMaxCams];
  for (int c = 0; c < n_cams; ++c) { in_tree[c] = false; cam_parent[c] = -1; cam_status[c] = kSeedRigNotConnected; }
  in_tree[0] = true; cam_status[0] = kSeedRigReached;
  for (int k = 0; k < 7; ++k) cam_T_c0[k] = k == 3 ? 1.0 : 0.0;
  for (;;) {
    int best = -1, bu = -1, bv = -1;
    for (int u = 0; u < n_cams; ++u) {
      if (!in_tree[u]) continue;
      for (int v = 0; v < n_cams; ++v) {
        if (in_tree[v]) continue;
        const int p = u < v ? srig_pair_index(n_cams, u, v) : srig_pair_index(n_cams, v, u);
        if (pair_status[p] == kSeedRigOk && pair_support[p] > best) { best = pair_support[p]; bu = u; bv = v; }     // (strictly more: the first of equals stays)
      }
    }
    if (bv < 0) break;
    double step[7];                                                    // camera bu into camera bv
    if (bu < bv) srig_pose_inv(pair_T_ab + 7 * (size_t)srig_pair_index(n_cams, bu, bv), step);
    else for (int k = 0; k < 7; ++k) step[k] = pair_T_ab[7 * (size_t)srig_pair_index(n_cams, bv, bu) + k];
    srig_pose_mul(step, cam_T_c0 + 7 * (size_t)bu, cam_T_c0 + 7 * (size_t)bv);
    in_tree[bv] = true; cam_parent[bv] = bu; cam_status[bv] = kSeedRigReached;
  }
}

}  // namespace vc
