#pragma once
// vc_target_refine.hpp -- the arithmetic of one Gauss-Newton step on the calibration target's points with the frame poses AND the shared
// camera columns marginalised (vc_target_refine_batch: include/vicalib_amd.h), shared by the kernels of vc_target_refine.hip and the host
// harness of the CPU tests (tests/host_harness/target_refine_harness.cpp).  VC_HD throughout, no HIP call.
//
//   rows of a corner, unit weight, no robust loss:  r = project(T_ck T_wk^-1 p) - z,  [J_f (2 x 6) | J_s (2 x camera's columns) | J_p (2 x 3)]
//     J_f, J_s: the rows of vc_select.hpp (sel_corner_rows, sel_view_blocks);  J_p = A R_cw, the derivative by the target point in the world
//   a frame with H_ff = L L^T (sel_chol6, its pivot rule and statuses) adds, with Y = L^-1 [J_f^T J_p | J_f^T J_s | J_f^T r],
//     J^T J - Y^T Y  and  -(J^T r - Y^T y_r)   to the system over [d (3P) | s (D)];   the corners of one point in one frame are ONE record: their
//     J_f^T J_p are summed (in camera order) before the solve, so that two cameras seeing the same dot both add to that dot's block
//   s is eliminated with the factorisation of diag(c) S_ss diag(c) + 1e-6 I, c_j = 1 / sqrt(S_ss[j][j]) (sel_scale, sel_chol_step)
//   over the observed points:  M = S + lambda I,  b = g - lambda Pi (points - nominal),  Q = the orthonormalised similarity tangent at
//     nominal about the observed centroid (tr_gauge_entry, modified Gram-Schmidt in that order, a column dropped at kTrGaugeTol),
//     (Pi M Pi + mu Q Q^T) d = Pi b,  mu = trace(M) / (3 P_obs),  refined = nominal + Pi (points - nominal) + d
#include "vc_select.hpp"

namespace vc {

constexpr int kTrMaxPoints = 1024, kTrMinPoints = 4;
constexpr int kTrMaxFrames = 1 << 20;             // the (frame, point) -> record table is n_frames x n_points ints: 4 GB at the two limits
constexpr int kTrNB = 32;                          // panel width of the dense factorisation
constexpr int kTrPad = 64;                         // the dense system's order is 3P rounded up to this (identity rows behind 3P)
constexpr double kTrPriorS = 1e-6;                 // on the scaled shared columns, as in 4.12
constexpr double kTrGaugeTol = 1e-9;               // a gauge column whose norm falls to this x its norm before orthogonalisation is dropped
constexpr double kTrPivotTol = 1e-12;              // a pivot of the dense factorisation <= this x the largest diagonal entry: singular
constexpr int kTrOk = 0, kTrSingular = 1;          // result status
constexpr int kTrPointOk = 0, kTrPointUnobserved = 1;
// a corner's record: F = J_f^T J_p (6 x 3), P = J_p^T J_p (3 x 3), g = J_p^T r (3), C = (J_s^T J_p)^T (3 x 16, the camera's own columns)
constexpr int kTrCornerF = 0, kTrCornerP = 18, kTrCornerG = 27, kTrCornerC = 32, kTrCornerStride = 80;
// a (frame, point) record: Y = L^-1 sum F (6 x 3), P (3 x 3, summed), g (3, summed)
constexpr int kTrRecY = 0, kTrRecP = 18, kTrRecG = 27, kTrRecStride = 32;
constexpr int kTrGaugeCols = 7;

VC_HD int tr_padded(int n_points) { return ((3 * n_points + kTrPad - 1) / kTrPad) * kTrPad; }

// the gradient of the unique columns beside sel_gram_add: acc[i] += row0[i] r0 + row1[i] r1
template <int MODEL>
VC_HD void tr_grad_add(const double* row0, const double* row1, double r0, double r1, double* acc /*sel_nu*/) {
  constexpr int nu = sel_nu(MODEL);
#if defined(__clang__)
#pragma unroll
#endif
  for (int i = 0; i < nu; ++i) acc[i] += row0[i] * r0 + row1[i] * r1;
}
// ... placed where gram_grad reads it, in the block sel_gram_expand has filled
template <int MODEL>
VC_HD void tr_grad_place(const double* acc, double* G /*kSelGramDoubles*/) {
  constexpr int nu = sel_nu(MODEL), nk = nu - 6;
  for (int i = 0; i < nu; ++i) {
    if (nk < 10) G[i * kUCols + 6 + nk] = acc[i]; else G[kGGrad + i] = acc[i];
  }
}
// The rows of a corner (sel_corner_rows) with its residual.  False for a corner at camera depth <= 0 (any model but kb4): it enters nothing.
template <int MODEL>
VC_HD bool tr_corner_rows(const TileXf& x, const double* K, const ModelPre& pre, const double* pw, const double* z, double* row0, double* row1, double* r /*2*/) {
  if (!sel_corner_rows<MODEL>(x, K, pre, pw, row0, row1)) return false;
  double pc[3], pix[2];
  tile_point(x, pw, pc);
  project_any<false>(MODEL, pc, K, pre, pix, nullptr, nullptr);
  r[0] = pix[0] - z[0]; r[1] = pix[1] - z[1];
  return true;
}
// a corner's record from its rows: J_f = [A V] diag(-R_ck, R_ck), J_s = [-V R_ck | A | B] as far as free, J_p = A R_cw
template <int MODEL>
VC_HD void tr_corner_record(const double* row0, const double* row1, const double* r, const double* Rck, const double* Rcw, int flags, double* out /*kTrCornerStride*/) {
  constexpr int nk = sel_nu(MODEL) - 6;
  double Jf[2][6], Js[2][kUCols], Jp[2][3];
  for (int i = 0; i < 2; ++i) {
    const double* row = i ? row1 : row0;
    for (int j = 0; j < 3; ++j) {
      Jf[i][j] = -(row[0] * Rck[j] + row[1] * Rck[3 + j] + row[2] * Rck[6 + j]);
      Jf[i][3 + j] = row[3] * Rck[j] + row[4] * Rck[3 + j] + row[5] * Rck[6 + j];
      Jp[i][j] = row[0] * Rcw[j] + row[1] * Rcw[3 + j] + row[2] * Rcw[6 + j];
    }
    int col = 0;
    if (flags & kCamRotFree) { for (int j = 0; j < 3; ++j) Js[i][col + j] = -Jf[i][3 + j]; col += 3; }
    if (flags & kCamTransFree) { for (int j = 0; j < 3; ++j) Js[i][col + j] = row[j]; col += 3; }
    if (flags & kCamKFree) { for (int k = 0; k < nk; ++k) Js[i][col + k] = row[6 + k]; col += nk; }
    for (int k = col; k < kUCols; ++k) Js[i][k] = 0.0;
  }
  for (int q = 0; q < 6; ++q)
    for (int j = 0; j < 3; ++j) out[kTrCornerF + q * 3 + j] = Jf[0][q] * Jp[0][j] + Jf[1][q] * Jp[1][j];
  for (int a = 0; a < 3; ++a) {
    for (int b = 0; b < 3; ++b) out[kTrCornerP + a * 3 + b] = Jp[0][a] * Jp[0][b] + Jp[1][a] * Jp[1][b];
    out[kTrCornerG + a] = Jp[0][a] * r[0] + Jp[1][a] * r[1];
    for (int k = 0; k < kUCols; ++k) out[kTrCornerC + a * kUCols + k] = Jp[0][a] * Js[0][k] + Jp[1][a] * Js[1][k];
  }
  for (int k = kTrCornerG + 3; k < kTrCornerC; ++k) out[k] = 0.0;
}
VC_HD void tr_corner_zero(double* out) { for (int k = 0; k < kTrCornerStride; ++k) out[k] = 0.0; }
// a (frame, point) record: adds one corner's F, P, g into sums (27 + 3 doubles in the record's layout, Y holding the sum of F until tr_record_solve)
VC_HD void tr_record_add(const double* corner, double* rec) {
  for (int k = 0; k < 18; ++k) rec[kTrRecY + k] += corner[kTrCornerF + k];
  for (int k = 0; k < 9; ++k) rec[kTrRecP + k] += corner[kTrCornerP + k];
  for (int k = 0; k < 3; ++k) rec[kTrRecG + k] += corner[kTrCornerG + k];
}
VC_HD void tr_record_solve(const double* L, const double* dinv, double* rec) {
  double F[18];
  for (int k = 0; k < 18; ++k) F[k] = rec[kTrRecY + k];
  for (int j = 0; j < 3; ++j) sel_schur_col(L, dinv, F, 3, j, rec + kTrRecY + j, 3);
}
// the block of records a and b of one frame in S_dd: -Y_a^T Y_b, entry (i, j) added to acc
VC_HD void tr_pair_sub(const double* Ya, const double* Yb, double* acc /*9*/) {
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) {
      double s = 0.0;
      for (int k = 0; k < 6; ++k) s += Ya[k * 3 + i] * Yb[k * 3 + j];
      acc[i * 3 + j] -= s;
    }
}
// y_a . v for a 6-vector or a column with stride ldv
VC_HD double tr_y_dot(const double* Y, int a, const double* v, int ldv) {
  double s = 0.0;
  for (int k = 0; k < 6; ++k) s += Y[k * 3 + a] * v[k * ldv];
  return s;
}
// One entry of z = U^-T v for the factor sel_chol_step leaves (upper triangle, pivots on the diagonal): z_k from z_0 .. z_k-1 (in zrow)
VC_HD double tr_fwd_entry(const double* U, int ld, int k, double vk, const double* zrow) {
  double s = vk;
  for (int i = 0; i < k; ++i) s -= U[i * ld + k] * zrow[i];
  return s / U[k * ld + k];
}
// entry a (0..2) of column c of the similarity tangent at a point u = nominal - centroid: translations, rotations e_k x u, scale
VC_HD double tr_gauge_entry(int c, int a, const double* u) {
  if (c < 3) return a == c ? 1.0 : 0.0;
  if (c == 6) return u[a];
  const int k = c - 3;
  const int a1 = (k + 1) % 3, a2 = (k + 2) % 3;      // e_k x u: component a1 = -u[a2], component a2 = u[a1]
  return a == a1 ? -u[a2] : a == a2 ? u[a1] : 0.0;
}
VC_HD bool tr_gauge_keep(double norm_after, double norm_before) { return norm_after > kTrGaugeTol * norm_before; }
VC_HD bool tr_pivot_ok(double d, double top) { return d > kTrPivotTol * top; }

}  // namespace vc
