// vc_uncertainty.hpp -- the arithmetic of mapping the projection uncertainty of one calibrated camera, shared by the kernels
// (vc_uncertainty.hip), the host entry points and the host harness of the CPU tests.  Camera A with intrinsics K (nk of them) and a covariance
// Cov of K, on the comparer's lattice (cmp_sample, vc_compare.hpp): the ray a_s of sample s is its pixel q_s through A's Newton inversion,
// scaled to unit length (the A half of cmp_rays).  B_s (2 x nk) and A_s (2 x 3) are the two blocks of project_any<true> at a_s;
// Jw_s = -A_s [a_s]x is the comparer's rotation row at R = I.  Over the fit set F -- inversion valid, rho <= fit_radius, a_z > 0 unless kb4 --
// G = sum Jw^T Jw (3 x 3), C = sum Jw^T B (3 x nk) and M = -G^-1 C: a change dK moves sample s by B_s dK, the rotation that best absorbs it over
// F is w = M dK, what is left is J_s dK with J_s = B_s + Jw_s M.  Sigma_s = J_s Cov J_s^T (Cov scaled by sigma_px^2 beforehand) is the 2 x 2
// covariance of the pixel shift the extrinsics cannot absorb.  Nothing here restates a camera formula.
#pragma once
#include "vc_convert.hpp"

struct vc_uncertainty;

namespace vc {

// one Gram sweep's sums: G packed (xx xy xz yy yz zz), C (3 x nk, row-major), size of the fit set
constexpr int unc_ngram(int nk) { return 6 + 3 * nk + 1; }
constexpr int kUncMaxGram = unc_ngram(10);       // 37
// the map sweep's summary: count, invalid, sum var, max lam, its sample; then per ring count, invalid, sum var, max lam
constexpr int kUncSumDoubles = 5, kUncRingDoubles = 4;
constexpr int unc_npacked(int nk) { return nk * (nk + 1) / 2; }

struct UncFit { double M[30]; };                 // 3 x nk, row-major: rad per unit of each parameter
struct UncCov { double P[55]; };                 // sigma_px^2 Cov, upper triangle row by row

// packed index of (r, s), r <= s, of an nk x nk symmetric matrix
constexpr int unc_pidx(int nk, int r, int s) { return r * nk - (r * (r - 1)) / 2 + (s - r); }

// The rows of one sample: B (2 x nk) and Jw (2 x 3) at the unit ray a.  false: a_z <= 0 and the model is not kb4.
template <int MODEL>
VC_HD bool unc_rows(const CmpPlan& p, const double* a, double* B, double* Jw) {
  if (!(a[2] > 0.0) && MODEL != kKb4) return false;
  double pix[2], A[6];
  project_any<true>(MODEL, a, p.Ka, p.pre_a, pix, A, B);
  const double x = a[0], y = a[1], z = a[2];
  // -A [a]x with [a]x = [0 -z y; z 0 -x; -y x 0]  (cmp_fit_sample's rows at R = I)
  Jw[0] = -(A[1] * z - A[2] * y); Jw[1] = -(A[2] * x - A[0] * z); Jw[2] = -(A[0] * y - A[1] * x);
  Jw[3] = -(A[4] * z - A[5] * y); Jw[4] = -(A[5] * x - A[3] * z); Jw[5] = -(A[3] * y - A[4] * x);
  return true;
}
// One sample of the Gram sweep: acc = [G packed | C] gets Jw^T Jw and Jw^T B.  false (acc untouched): the sample is not in F.
// Every index is a constant once the loops are unrolled: the sums stay in registers.
template <int MODEL>
VC_HD bool unc_gram_sample(const CmpPlan& p, const double* a, double* acc) {
  constexpr int nk = cvt_nk(MODEL);
  double B[20], Jw[6];
  if (!unc_rows<MODEL>(p, a, B, Jw)) return false;
  acc[0] += Jw[0] * Jw[0] + Jw[3] * Jw[3]; acc[1] += Jw[0] * Jw[1] + Jw[3] * Jw[4]; acc[2] += Jw[0] * Jw[2] + Jw[3] * Jw[5];
  acc[3] += Jw[1] * Jw[1] + Jw[4] * Jw[4]; acc[4] += Jw[1] * Jw[2] + Jw[4] * Jw[5]; acc[5] += Jw[2] * Jw[2] + Jw[5] * Jw[5];
#if defined(__clang__)
#pragma unroll
#endif
  for (int i = 0; i < 3; ++i) {
#if defined(__clang__)
#pragma unroll
#endif
    for (int k = 0; k < nk; ++k) acc[6 + i * nk + k] += Jw[i] * B[k] + Jw[3 + i] * B[nk + k];
  }
  return true;
}
// Sigma = J P J^T of one sample with J = B + Jw M: s = (s_uu, s_uv, s_vv).  false: the rows do not exist (unc_rows) or Sigma is not finite.
template <int MODEL>
VC_HD bool unc_sigma_sample(const CmpPlan& p, const double* a, const UncFit& fit, const UncCov& cov, double* s) {
  constexpr int nk = cvt_nk(MODEL);
  double B[20], Jw[6];
  if (!unc_rows<MODEL>(p, a, B, Jw)) return false;
#if defined(__clang__)
#pragma unroll
#endif
  for (int k = 0; k < nk; ++k) {
    B[k] += Jw[0] * fit.M[k] + Jw[1] * fit.M[nk + k] + Jw[2] * fit.M[2 * nk + k];
    B[nk + k] += Jw[3] * fit.M[k] + Jw[4] * fit.M[nk + k] + Jw[5] * fit.M[2 * nk + k];
  }
  double uu = 0.0, uv = 0.0, vv = 0.0;
#if defined(__clang__)
#pragma unroll
#endif
  for (int k = 0; k < nk; ++k) {
    double t0 = 0.0, t1 = 0.0;                                   // row k of P against the two rows of J
#if defined(__clang__)
#pragma unroll
#endif
    for (int l = 0; l < nk; ++l) {
      const double c = cov.P[k <= l ? unc_pidx(nk, k, l) : unc_pidx(nk, l, k)];
      t0 += c * B[l]; t1 += c * B[nk + l];
    }
    uu += B[k] * t0; uv += B[k] * t1; vv += B[nk + k] * t1;
  }
  s[0] = uu; s[1] = uv; s[2] = vv;
  return fabs(uu) <= 1e300 && fabs(uv) <= 1e300 && fabs(vv) <= 1e300;      // (a NaN fails the comparison)
}
// var = s_uu + s_vv, the expected squared shift; lam = the larger eigenvalue of Sigma, clamped at 0: the variance along the worst direction
VC_HD double unc_var(const double* s) { return s[0] + s[2]; }
VC_HD double unc_lam(const double* s) {
  const double df = s[0] - s[2];
  const double l = 0.5 * ((s[0] + s[2]) + sqrt(df * df + 4.0 * (s[1] * s[1])));
  return l > 0.0 ? l : 0.0;
}

// ---- host side --------------------------------------------------------------------------------------------------------------------
// a run's covariance and noise scale: every entry finite, symmetric to 1e-12 max |diag|, no negative diagonal entry, sigma_px > 0 and finite
inline bool unc_run_args_ok(const double* cov, int nk, double sigma_px, double fit_radius) {
  if (!cov || !(sigma_px > 0.0) || !(sigma_px <= 1e300) || !(fit_radius == fit_radius) || !(fabs(fit_radius) <= 1e300)) return false;
  double dmax = 0.0;
  for (int k = 0; k < nk * nk; ++k) if (!(fabs(cov[k]) <= 1e300)) return false;
  for (int k = 0; k < nk; ++k) {
    if (cov[k * nk + k] < 0.0) return false;
    dmax = fmax(dmax, cov[k * nk + k]);
  }
  for (int r = 0; r < nk; ++r)
    for (int s = r + 1; s < nk; ++s) if (!(fabs(cov[r * nk + s] - cov[s * nk + r]) <= 1e-12 * dmax)) return false;
  return true;
}
// P = sigma_px^2 Cov, packed; the mean of the two halves where they differ within the tolerance.  The scaling comes before the sweep: with
// sigma_px doubled every product of the sweep is the same product times four.
inline void unc_pack_cov(const double* cov, int nk, double sigma_px, UncCov* out) {
  const double s2 = sigma_px * sigma_px;
  for (int k = 0; k < 55; ++k) out->P[k] = 0.0;
  for (int r = 0; r < nk; ++r)
    for (int s = r; s < nk; ++s) out->P[unc_pidx(nk, r, s)] = s2 * (0.5 * (cov[r * nk + s] + cov[s * nk + r]));
}
// M = -G^-1 C from one Gram sweep's sums; G9 = G in full.  false: fewer than 3 samples in F or a G without a positive pivot.
inline bool unc_solve_fit(const double* sums, int nk, UncFit* fit, double* G9, long long* n_fit) {
  const double* g = sums;
  *n_fit = (long long)sums[6 + 3 * nk];
  const double G[9] = {g[0], g[1], g[2], g[1], g[3], g[4], g[2], g[4], g[5]};
  for (int k = 0; k < 9; ++k) G9[k] = G[k];
  for (int k = 0; k < 30; ++k) fit->M[k] = 0.0;
  if (*n_fit < 3) return false;
  double L[9];
  for (int k = 0; k < 9; ++k) L[k] = G[k];
  if (!chol_small<3>(L)) return false;
  for (int k = 0; k < nk; ++k) {
    double x[3] = {-sums[6 + k], -sums[6 + nk + k], -sums[6 + 2 * nk + k]};
    fwd_solve<3>(L, x); bwd_solve<3>(L, x);
    for (int i = 0; i < 3; ++i) {
      if (!(fabs(x[i]) <= 1e300)) return false;
      fit->M[i * nk + k] = x[i];
    }
  }
  return true;
}

// the calibrator's covariance of a handle made by vc_uncertainty_create_for_camera (nk x nk, copied)
void unc_attach_cov(vc_uncertainty* u, const double* cov);

}  // namespace vc
