#pragma once
// vc_select.hpp -- the arithmetic of greedy D-optimal view selection (vc_selector: include/vicalib_amd.h), shared by the kernels of
// vc_select.hip and the host harness of the CPU tests (tests/host_harness/select_harness.cpp).  VC_HD throughout, no HIP call.
//
//   information of frame f on the D shared columns [w_ck | t_ck | K] per camera as far as free, its pose marginalised, at unit weight:
//     I_f = J_s^T J_s - J_s^T J_f (J_f^T J_f)^-1 J_f^T J_s          (packed upper triangle, row by row: sel_pack_idx)
//   scale   s_j = 1 / sqrt(sum_f I_f[j][j]) over usable frames (1 where the sum is 0),  I~_f = diag(s) I_f diag(s)
//   gain    logdet(S + I~_f) - logdet(S) = sum_k log(p'_k / p_k) over the pivots of the two Cholesky factorisations: S + I~_f >= S, so
//           every p'_k >= p_k and no two large logarithms are subtracted
//   pick    the largest gain, the lowest frame on exactly equal gains (sel_better)
#include "vc_math.hpp"

namespace vc {

constexpr int kSelMaxCams = 8, kSelMaxD = 64;
constexpr int kSelUsable = 0, kSelUnderdetermined = 1, kSelBehind = 2;      // frame status
constexpr double kSelPivotTol = 1e-12;                                        // a pivot of J_f^T J_f <= this x its largest diagonal entry: underdetermined
constexpr int kSelGramDoubles = kGGrad + kUCols;                              // a view's 16 x 16 Gram block + the (zero) side vector the block functions read

// the rig as the kernels take it: camera records [T_ck (7) pad | K (10) pad] and the layout of the shared columns
struct SelRig {
  int n_cams, D;
  int model[kSelMaxCams], flags[kSelMaxCams], col0[kSelMaxCams], ncols[kSelMaxCams];
  double cam[kSelMaxCams * kCamStride];
};
// fills col0 / ncols / D from model and flags; false beyond kSelMaxD (the caller reports VC_ERR_UNSUPPORTED)
VC_HD bool sel_layout(SelRig* r) {
  int d = 0;
  for (int c = 0; c < r->n_cams; ++c) { r->col0[c] = d; r->ncols[c] = cam_ncols(r->flags[c], model_nk(r->model[c])); d += r->ncols[c]; }
  r->D = d;
  return d <= kSelMaxD;
}
VC_HD int sel_col_cam(const SelRig& r, int col) {
  int c = 0;
  for (int k = 1; k < r.n_cams; ++k) if (col >= r.col0[k]) c = k;
  return c;
}

VC_HD int sel_pack_len(int D) { return D * (D + 1) / 2; }
VC_HD int sel_pack_idx(int i, int j, int D) { return i * D - (i * (i - 1)) / 2 + (j - i); }      // i <= j

constexpr int sel_nu(int model) { return 6 + (model == kFov ? 5 : model == kPoly2 ? 6 : model == kPoly3 ? 7 : model == kKb4 ? 8 : model == kRational6 ? 10 : 4); }
constexpr int sel_nacc(int model) { return sel_nu(model) * (sel_nu(model) + 1) / 2; }

// The two rows [A_i | A_i x q | B_i] of one corner at unit weight (no measurement, no robust loss).  False for a corner at camera depth
// <= 0 (any model but kb4): it enters no sum.
template <int MODEL>
VC_HD bool sel_corner_rows(const TileXf& x, const double* K, const ModelPre& pre, const double* pw, double* row0 /*16*/, double* row1 /*16*/) {
  constexpr int nk = sel_nu(MODEL) - 6;
  double pc[3], pix[2], A[6], B[20];
  tile_point(x, pw, pc);
  if (MODEL != kKb4 && !(pc[2] > 0.0)) return false;
  project_any<true>(MODEL, pc, K, pre, pix, A, B);
  const double q0 = pc[0] - x.tck[0], q1 = pc[1] - x.tck[1], q2 = pc[2] - x.tck[2];
  for (int i = 0; i < 2; ++i) {
    double* row = i ? row1 : row0;
    const double* a = A + 3 * i;
    row[0] = a[0]; row[1] = a[1]; row[2] = a[2];
    row[3] = a[1] * q2 - a[2] * q1;
    row[4] = a[2] * q0 - a[0] * q2;
    row[5] = a[0] * q1 - a[1] * q0;
    for (int k = 0; k < nk; ++k) row[6 + k] = B[i * nk + k];
    for (int k = 6 + nk; k < kUCols; ++k) row[k] = 0.0;
  }
  return true;
}
// a corner's share of the view's Gram sums: the upper triangle over the 6 + nk columns, row by row
template <int MODEL>
VC_HD void sel_gram_add(const double* row0, const double* row1, double* acc /*sel_nacc*/) {
  constexpr int nu = sel_nu(MODEL);
  int e = 0;
#if defined(__clang__)
#pragma unroll
#endif
  for (int i = 0; i < nu; ++i)
#if defined(__clang__)
#pragma unroll
#endif
    for (int j = i; j < nu; ++j) { acc[e] += row0[i] * row0[j] + row1[i] * row1[j]; ++e; }
}
// ... expanded to the symmetric 16 x 16 block the block functions take (the side vector zero: there is no residual)
template <int MODEL>
VC_HD void sel_gram_expand(const double* acc, double* G /*kSelGramDoubles*/) {
  constexpr int nu = sel_nu(MODEL);
  for (int k = 0; k < kSelGramDoubles; ++k) G[k] = 0.0;
  int e = 0;
  for (int i = 0; i < nu; ++i)
    for (int j = i; j < nu; ++j) { G[i * kUCols + j] = acc[e]; G[j * kUCols + i] = acc[e]; ++e; }
}
// a view's blocks from its Gram block: Hff (6 x 6, adds), W (6 x ncols, ld 16) and the camera's own block Hcc (ncols x ncols, ld 16)
VC_HD void sel_view_blocks(const double* G, const double* T_ck, int model, int flags, double* Hff /*36*/, double* W /*96*/, double* Hcc /*256*/,
                           double* tmp /*22: gf, gc*/) {
  double R[9];
  quat_to_R(T_ck, R);
  const int nk = model_nk(model);
  tile_to_frame_blocks(G, R, nk, flags, Hff, tmp, W);
  cam_block_from_gsum(G, R, nk, flags, Hcc, tmp + 6);
}
// 6 x 6 in-place lower Cholesky of J_f^T J_f with the pivot rule of the frame status; dinv[j] = 1 / L[j][j]
VC_HD bool sel_chol6(double* M /*36*/, double* dinv /*6*/) {
  double top = 0.0;
  for (int j = 0; j < 6; ++j) top = M[j * 6 + j] > top ? M[j * 6 + j] : top;
  const double floor_ = kSelPivotTol * top;
  for (int j = 0; j < 6; ++j) {
    double d = M[j * 6 + j];
    for (int k = 0; k < j; ++k) d -= M[j * 6 + k] * M[j * 6 + k];
    if (!(d > floor_)) return false;
    const double l = sqrt(d), id = 1.0 / l;
    M[j * 6 + j] = l; dinv[j] = id;
    for (int i = j + 1; i < 6; ++i) {
      double s = M[i * 6 + j];
      for (int k = 0; k < j; ++k) s -= M[i * 6 + k] * M[j * 6 + k];
      M[i * 6 + j] = s * id;
    }
  }
  return true;
}
// y = L^-1 W[:, j]  (W with leading dimension ldw; y with stride ldy)
VC_HD void sel_schur_col(const double* L, const double* dinv, const double* W, int ldw, int j, double* y, int ldy) {
  double t[6];
  for (int i = 0; i < 6; ++i) {
    double s = W[i * ldw + j];
    for (int k = 0; k < i; ++k) s -= L[i * 6 + k] * t[k];
    t[i] = s * dinv[i];
  }
  for (int i = 0; i < 6; ++i) y[i * ldy] = t[i];
}
// I_f[i][j] = Hss[i][j] - y_i . y_j
VC_HD double sel_info_entry(double hss, const double* Y, int ldy, int i, int j) {
  double s = 0.0;
  for (int k = 0; k < 6; ++k) s += Y[k * ldy + i] * Y[k * ldy + j];
  return hss - s;
}
VC_HD int sel_frame_status(int corners, int behind, bool chol_ok) {
  if (corners < 4 || !chol_ok) return kSelUnderdetermined;
  return behind > 0 ? kSelBehind : kSelUsable;
}
VC_HD bool sel_usable(int status) { return status != kSelUnderdetermined; }

VC_HD double sel_scale(double diag_sum) { return diag_sum > 0.0 ? 1.0 / sqrt(diag_sum) : 1.0; }
VC_HD double sel_scaled(double I, double si, double sj) { return (si * I) * sj; }

// One step of the in-place factorisation of a symmetric positive definite M (upper triangle, leading dimension ld), lane = column: with
// pivot k final, column j > k takes its update of rows k + 1 .. j.  The steps of one k are independent of each other; those of k + 1 follow
// those of k.  Afterwards M[k][k], k = 0 .. D-1, are the pivots: logdet = sum log.
VC_HD void sel_chol_step(double* M, int ld, int k, int j) {
  const double f = M[k * ld + j] / M[k * ld + k];
  for (int i = k + 1; i <= j; ++i) M[i * ld + j] -= M[k * ld + i] * f;
}
// a pivot's share of logdet(S') - logdet(S)
VC_HD double sel_gain_term(double p_new, double p_old) { return log(p_new / p_old); }
// the pick rule: a larger gain wins, the lower frame on exactly equal gains
VC_HD bool sel_better(double gain, int frame, double best, int best_frame) {
  return gain > best || (gain == best && frame >= 0 && (best_frame < 0 || frame < best_frame));
}
VC_HD bool sel_prior_ok(double prior) { return prior > 0.0 && prior < 1e300; }      // finite and positive (NaN fails both)

}  // namespace vc
