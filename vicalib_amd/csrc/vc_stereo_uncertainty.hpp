// vc_stereo_uncertainty.hpp -- the arithmetic of mapping the row and depth uncertainty of a calibrated stereo pair, shared by the kernels
// (vc_stereo_uncertainty.hip), the host entry points and the host harness of the CPU tests.  Cameras A and B with their intrinsics and
// poses, the rectified frames of rectify_rotations (vc_rectify.hpp) and a FIXED destination pinhole dl = (fu, fv, u0, v0) of dst_w x dst_h.
// A sample is a point (x, y) of the comparer's lattice (cmp_sample, vc_compare.hpp) over the rectified image of A with a depth Z > 0:
//   P = ((x - u0) Z / fu, (y - v0) Z / fv, Z) in A's rectified frame, P - (b, 0, 0) in B's; the rays a = R_ds_a^T P, bb = R_ds_b^T (P - (b, 0, 0))
// and the pixels p_a, p_b they are seen at, with A (2 x 3) and B (2 x nk) of project_any<true>.  A user holding another calibration pushes
// those fixed pixels through rectify_pair's arithmetic.  Per side, to first order: the ray of the fixed pixel moves by
// da = -A^T (A A^T)^-1 B dK (A a = 0: the component along the ray is free and the pinhole step drops it), the rectified ray r = R_ds a by
// dr = R_ds da - [r]x w when R_ds moves as exp([w]x) R_ds, and the rectified pixel by Pi(r) dr with
// Pi = [[fu / r_z, 0, -fu r_x / r_z^2], [0, fv / r_z, -fv r_y / r_z^2]]: the side's block [-Pi [r]x | Pi R_ds da/dK], 2 x (3 + nk).
// Over eta = [w_a (3), w_b (3), db, dK_a (10), dK_b (10)] (27, unused intrinsics zero) the three rows of a sample are
//   dv = v_a - v_b,  d = u_a - u_b,  Z: (fu / d) db - (Z / d) d(d) with d = fu b / Z,
// and what is stored is row Cov_eta row^T for each: (var_dv, var_d, var_Z) in px^2, px^2, m^2.  Cov_eta = T Cov T^T is formed on the host
// (su_pack_cov) from the covariance of a two-camera rig in vc_get_solution_covariance's layout.  Nothing here restates a camera formula.
#pragma once
#include "vc_uncertainty.hpp"

struct vc_stereo_uncertainty;

namespace vc {

constexpr int kSuMaxDepths = 8;                  // depth planes of one run
constexpr int kSuSideCols = 13;                  // a side's block: 3 rotation columns, 10 intrinsics (zero from nk on)
constexpr int kSuSideDoubles = 2 * kSuSideCols;  // row u, then row v
constexpr int kSuEta = 27;                       // w_a (3), w_b (3), db, dK_a (10), dK_b (10)
constexpr int kSuPacked = kSuEta * (kSuEta + 1) / 2;      // 378
// a depth plane's summary: count, invalid, sum var_dv, sum var_d, sum var_Z, max var_dv, its sample
constexpr int kSuSumDoubles = 7;
constexpr int kSuMaxCov = 14 + 20;               // q (4) p (3) K (<= 10) per camera

struct SuCov { double P[kSuPacked]; };           // sigma_px^2 Cov_eta, upper triangle row by row
constexpr int su_pidx(int r, int s) { return r * kSuEta - (r * (r - 1)) / 2 + (s - r); }

struct SuPlan {
  CmpPlan lat;               // the lattice over the rectified image (w, h = the destination's) and the two cameras' models and intrinsics
  int src_w[2], src_h[2];
  double dl[4];              // the destination pinhole
  double R_ds[2][9];
  double baseline;
};

// the point of lattice sample s at depth Z in the rectified frame of side `side`
VC_HD void su_point(const SuPlan& p, int s, double Z, int side, double* r) {
  double x, y, rho;
  cmp_sample(p.lat, s, &x, &y, &rho);
  r[0] = (x - p.dl[2]) * Z / p.dl[0] - (side ? p.baseline : 0.0);
  r[1] = (y - p.dl[3]) * Z / p.dl[1];
  r[2] = Z;
}

// One side of one sample: blk = [-Pi [r]x | Pi R_ds da/dK] as row u (13), row v (13) at the rectified point r.  false (blk untouched): the
// ray has z <= 0 in the camera (unless kb4), its pixel is not finite or outside [0, w - 1] x [0, h - 1], or A A^T has no inverse.
template <int MODEL>
VC_HD bool su_side_block(const double* K, const ModelPre& pre, int w, int h, const double* R_ds, const double* dl, const double* r, double* blk) {
  constexpr int nk = cvt_nk(MODEL);
  const double a[3] = {R_ds[0] * r[0] + R_ds[3] * r[1] + R_ds[6] * r[2], R_ds[1] * r[0] + R_ds[4] * r[1] + R_ds[7] * r[2],
                       R_ds[2] * r[0] + R_ds[5] * r[1] + R_ds[8] * r[2]};
  if (!(a[2] > 0.0) && MODEL != kKb4) return false;
  double pix[2], A[6], B[20];
  project_any<true>(MODEL, a, K, pre, pix, A, B);
  if (!(pix[0] >= 0.0 && pix[0] <= (double)(w - 1) && pix[1] >= 0.0 && pix[1] <= (double)(h - 1))) return false;      // (a NaN fails the chain)
  const double s00 = A[0] * A[0] + A[1] * A[1] + A[2] * A[2], s01 = A[0] * A[3] + A[1] * A[4] + A[2] * A[5], s11 = A[3] * A[3] + A[4] * A[4] + A[5] * A[5];
  const double det = s00 * s11 - s01 * s01;
  if (!(det > 0.0) || !(det <= 1e300)) return false;
  const double i00 = s11 / det, i01 = -s01 / det, i11 = s00 / det;
  // D = Pi R_ds A^T (A A^T)^-1, 2 x 2: the rectified pixel per unit of pixel shift in the camera; the K columns are -D B
  const double rz = 1.0 / r[2];
  const double pu[3] = {dl[0] * rz, 0.0, -dl[0] * r[0] * rz * rz}, pv[3] = {0.0, dl[1] * rz, -dl[1] * r[1] * rz * rz};
  double g[6];                                                       // R_ds A^T (A A^T)^-1, 3 x 2
#if defined(__clang__)
#pragma unroll
#endif
  for (int i = 0; i < 3; ++i) {
    const double ra0 = R_ds[3 * i] * A[0] + R_ds[3 * i + 1] * A[1] + R_ds[3 * i + 2] * A[2];
    const double ra1 = R_ds[3 * i] * A[3] + R_ds[3 * i + 1] * A[4] + R_ds[3 * i + 2] * A[5];
    g[2 * i] = ra0 * i00 + ra1 * i01; g[2 * i + 1] = ra0 * i01 + ra1 * i11;
  }
  const double d00 = pu[0] * g[0] + pu[2] * g[4], d01 = pu[0] * g[1] + pu[2] * g[5];
  const double d10 = pv[1] * g[2] + pv[2] * g[4], d11 = pv[1] * g[3] + pv[2] * g[5];
  // -p^T [r]x with [r]x = [0 -z y; z 0 -x; -y x 0]
  blk[0] = -(pu[1] * r[2] - pu[2] * r[1]); blk[1] = -(pu[2] * r[0] - pu[0] * r[2]); blk[2] = -(pu[0] * r[1] - pu[1] * r[0]);
  blk[kSuSideCols] = -(pv[1] * r[2] - pv[2] * r[1]); blk[kSuSideCols + 1] = -(pv[2] * r[0] - pv[0] * r[2]); blk[kSuSideCols + 2] = -(pv[0] * r[1] - pv[1] * r[0]);
#if defined(__clang__)
#pragma unroll
#endif
  for (int k = 0; k < 10; ++k) {
    blk[3 + k] = k < nk ? -(d00 * B[k] + d01 * B[nk + k]) : 0.0;
    blk[kSuSideCols + 3 + k] = k < nk ? -(d10 * B[k] + d11 * B[nk + k]) : 0.0;
  }
  return true;
}

// The three variances of one sample from the two sides' blocks in ONE pass over the packed symmetric P.  The rows of dv (the v rows) and of d
// (the u rows) have no entry at db (index 6), and the row of Z is zd (row of d) + g e_6 with zd = -Z / d, g = fu / d, so
//   var_dv = jv^T P jv,  var_d = ju^T P ju,  var_Z = zd^2 var_d + 2 zd g (P ju)_6 + g^2 P_66:
// every entry of P is read once and meets both rows -- 377 reads where three quadratic forms of their own take 1134 (and the compiler, which
// sees the same 378 addresses three times, keeps them in registers between the forms and spills).  Every index is a constant once the loops
// are unrolled: the rows stay in registers and P is read at addresses that do not depend on the sample.  false: a variance is not finite.
VC_HD bool su_variances(const double* ba, const double* bb, double fu, double Z, double baseline, const double* P, double* var) {
  double ju[kSuEta], jv[kSuEta];
#if defined(__clang__)
#pragma unroll
#endif
  for (int k = 0; k < 3; ++k) { ju[k] = ba[k]; ju[3 + k] = -bb[k]; jv[k] = ba[kSuSideCols + k]; jv[3 + k] = -bb[kSuSideCols + k]; }
  ju[6] = 0.0; jv[6] = 0.0;
#if defined(__clang__)
#pragma unroll
#endif
  for (int k = 0; k < 10; ++k) { ju[7 + k] = ba[3 + k]; ju[17 + k] = -bb[3 + k]; jv[7 + k] = ba[kSuSideCols + 3 + k]; jv[17 + k] = -bb[kSuSideCols + 3 + k]; }
  double qu = 0.0, qv = 0.0, c6 = 0.0;                               // c6 = (P ju)_6
#if defined(__clang__)
#pragma unroll
#endif
  for (int k = 0; k < kSuEta; ++k) {
    double tu = 0.0, tv = 0.0;
#if defined(__clang__)
#pragma unroll
#endif
    for (int l = k + 1; l < kSuEta; ++l) {
      const double p = P[su_pidx(k, l)];
      if (l == 6) c6 += p * ju[k];                                   // (column 6 meets no row entry: ju_6 = jv_6 = 0)
      else { tu += p * ju[l]; tv += p * jv[l]; }
    }
    if (k == 6) c6 += tu;
    else {
      const double pkk = P[su_pidx(k, k)];
      qu += ju[k] * (pkk * ju[k] + 2.0 * tu); qv += jv[k] * (pkk * jv[k] + 2.0 * tv);
    }
  }
  const double d = fu * baseline / Z, zd = -Z / d, g = fu / d;
  var[0] = qv; var[1] = qu;
  var[2] = zd * zd * qu + 2.0 * (zd * g) * c6 + g * g * P[su_pidx(6, 6)];
  return fabs(var[0]) <= 1e300 && fabs(var[1]) <= 1e300 && fabs(var[2]) <= 1e300;      // (a NaN fails the comparison)
}

// ---- host side --------------------------------------------------------------------------------------------------------------------
// a run's arguments: the covariance as unc_run_args_ok holds one (n = 14 + nk_a + nk_b), 1 to 8 depths, each > 0 and finite
inline bool su_run_args_ok(const double* cov, int n, double sigma_px, const double* depths, int n_depths) {
  if (!depths || n_depths < 1 || n_depths > kSuMaxDepths || !unc_run_args_ok(cov, n, sigma_px, 0.0)) return false;
  for (int k = 0; k < n_depths; ++k) if (!(depths[k] > 0.0) || !(depths[k] <= 1e300)) return false;
  return true;
}
// T (27 x n): eta per unit of the ambient parameters [q_a (4) p_a (3) K_a q_b (4) p_b (3) K_b].  The tangent rotation of a pose is
// w_ck = 2 J^T dq with J the 4 x 3 matrix of vc_get_solution_covariance (dq = 1/2 J w_ck, J^T J = I for a unit quaternion); then
// (w_a, w_b, db) = W [w_ck_a, dp_a, w_ck_b, dp_b] with W of rect_pose_jacobian; the intrinsics pass through.
inline void su_eta_map(const double* T_ck_a, const double* T_ck_b, int nka, int nkb, const double* W, double* T) {
  const int n = 14 + nka + nkb;
  for (int k = 0; k < kSuEta * n; ++k) T[k] = 0.0;
  const double* Tck[2] = {T_ck_a, T_ck_b};
  const int first[2] = {0, 7 + nka};
  for (int c = 0; c < 2; ++c) {
    const double* q = Tck[c];
    const double J[12] = {q[3], -q[2], q[1], q[2], q[3], -q[0], -q[1], q[0], q[3], -q[0], -q[1], -q[2]};
    for (int i = 0; i < 7; ++i) {
      for (int r = 0; r < 4; ++r)
        for (int a = 0; a < 3; ++a) T[i * n + first[c] + r] += W[i * 12 + 6 * c + a] * 2.0 * J[3 * r + a];
      for (int a = 0; a < 3; ++a) T[i * n + first[c] + 4 + a] = W[i * 12 + 6 * c + 3 + a];
    }
  }
  for (int k = 0; k < nka; ++k) T[(7 + k) * n + 7 + k] = 1.0;
  for (int k = 0; k < nkb; ++k) T[(17 + k) * n + first[1] + 7 + k] = 1.0;
}
// P = sigma_px^2 T Cov T^T, packed.  Cov is symmetrised (the mean of its two halves) and scaled before the products: with sigma_px doubled
// every product here and in the sweep is the same product times four.
inline void su_pack_cov(const double* cov, int n, const double* T, double sigma_px, SuCov* out) {
  const double s2 = sigma_px * sigma_px;
  double C[kSuMaxCov * kSuMaxCov], TC[kSuEta * kSuMaxCov];
  for (int r = 0; r < n; ++r)
    for (int s = 0; s < n; ++s) C[r * n + s] = s2 * (0.5 * (cov[r * n + s] + cov[s * n + r]));
  for (int i = 0; i < kSuEta; ++i)
    for (int s = 0; s < n; ++s) {
      double t = 0.0;
      for (int r = 0; r < n; ++r) t += T[i * n + r] * C[r * n + s];
      TC[i * n + s] = t;
    }
  for (int i = 0; i < kSuEta; ++i)
    for (int k = i; k < kSuEta; ++k) {
      double t = 0.0, u = 0.0;
      for (int s = 0; s < n; ++s) { t += TC[i * n + s] * T[k * n + s]; u += TC[k * n + s] * T[i * n + s]; }
      out->P[su_pidx(i, k)] = 0.5 * (t + u);
    }
}

// the calibrator's covariance of a handle made by vc_stereo_uncertainty_create_for_cameras (n x n, copied)
void su_attach_cov(vc_stereo_uncertainty* u, const double* cov);

}  // namespace vc
