// vc_convert.hpp -- the arithmetic of converting a calibrated camera to another camera model, shared by the kernels (vc_convert.hip), the host
// entry points and the host harness of the CPU tests.  Source camera A, target model m_b, and the comparer's lattice (cmp_sample,
// vc_compare.hpp): the ray a_s of sample s is its pixel q_s through A's Newton inversion (undist_unproject, vc_undistort.hpp), scaled to unit
// length.  Over the fit set F -- the samples whose inversion succeeded and whose rho <= fit_radius -- the intrinsics K_b of model m_b
// minimise E(K_b) = sum |project(m_b, K_b, a_s) - q_s|^2: the rows are block B of project_any<true> (vc_math.hpp), the closed-form Jacobian
// with respect to the intrinsics.  No rotation and no extrinsics: the converted camera sees the same rays.  Levenberg-Marquardt runs on the
// host over sweeps of the samples, with the project's rules (LmRules, lm_clamped_diag, chol_small).  Nothing here restates a camera formula.
#pragma once
#include "vc_compare.hpp"
#include "vc_lm_rules.hpp"

namespace vc {

enum { kCvtFlagA = 1, kCvtFlagOutside = 2 };      // a sample's flag byte: A's inversion failed; rho > fit_radius.  0: the sample is in F.
enum { kCvtConverged = 0, kCvtMaxItersReached = 1, kCvtFailed = 2 };
constexpr int kCvtDefaultIters = 50, kCvtMaxIters = 200;
constexpr double kCvtStepTol = 1e-10, kCvtCostTol = 1e-12;
// the reference's own starting value of the fov model's w (vicalib-engine.cc:207).  Not 0: project_radial takes fac = 1 for w^2 <= 1e-5 and
// gives d fac / d w = 0 there by construction, so the column of w would be zero and w, pinned by the damping alone, would never leave 0.
constexpr double kCvtFovStart = 0.2;

// one linearisation's sums: J^T J packed (upper triangle row by row, nk (nk + 1) / 2), J^T d (nk), E, samples used, samples of F left out
constexpr int cvt_nk(int m) { return m == kFov ? 5 : m == kPoly2 ? 6 : m == kPoly3 ? 7 : m == kKb4 ? 8 : m == kRational6 ? 10 : 4; }
constexpr int cvt_nh(int nk) { return nk * (nk + 1) / 2; }
constexpr int cvt_nsums(int nk) { return cvt_nh(nk) + nk + 3; }
constexpr int kCvtMaxSums = cvt_nsums(10);       // 68
// a cost sweep's record: E, used, left out, the largest |d|^2 (cmp_norm2) over the samples used and its sample (the lowest of equal ones; -1, -1: none)
constexpr int kCvtCostDoubles = 5;

// the target camera at one point of the fit
struct CvtCam { double K[10]; ModelPre pre; };
inline void cvt_cam(int model_b, const double* K, CvtCam* c) {
  const int nk = model_nk(model_b);
  for (int k = 0; k < 10; ++k) c->K[k] = k < nk ? K[k] : 0.0;
  model_precompute(model_b, c->K, &c->pre);
}

// A's inversion of one sample: a of unit length, or zero with kCvtFlagA (the A half of cmp_rays, in its arithmetic)
VC_HD int cvt_ray(const CmpPlan& p, double qx, double qy, double* a) {
  if (!undist_unproject(p.model_a, p.Ka, p.pre_a, qx, qy, a)) { a[0] = a[1] = a[2] = 0.0; return kCvtFlagA; }
  const double in = 1.0 / sqrt(a[0] * a[0] + a[1] * a[1] + a[2] * a[2]); a[0] *= in; a[1] *= in; a[2] *= in;
  return 0;
}
// d = project(m_b, K_b, a) - q and, with JAC, block B (2 x nk, row-major); false by the rule of cmp_project: a_z <= 0 (not kb4) or d is not finite
template <int MODEL, bool JAC>
VC_HD bool cvt_project(const CvtCam& c, const double* a, double qx, double qy, double* d, double* B) {
  if (!(a[2] > 0.0) && MODEL != kKb4) return false;
  double pix[2], A[6];
  project_any<JAC>(MODEL, a, c.K, c.pre, pix, A, B);
  d[0] = pix[0] - qx; d[1] = pix[1] - qy;
  return fabs(d[0]) <= 1e300 && fabs(d[1]) <= 1e300;         // (a NaN fails the comparison)
}
// One sample of a linearisation at K_b: the rows J = B and d are added to acc = [J^T J packed | J^T d | E].  false (acc untouched): the sample
// is left out at this K_b.  Every index is a constant once the loops are unrolled: the sums stay in registers.  (The two counts are the
// caller's own variables: one of two array elements incremented behind a branch becomes one increment at a selected address, in scratch.)
template <int MODEL>
VC_HD bool cvt_fit_sample(const CvtCam& c, const double* a, double qx, double qy, double* acc) {
  constexpr int nk = cvt_nk(MODEL), nh = cvt_nh(nk);
  double d[2], B[20];
  if (!cvt_project<MODEL, true>(c, a, qx, qy, d, B)) return false;
  int k = 0;
#if defined(__clang__)
#pragma unroll
#endif
  for (int r = 0; r < nk; ++r) {
#if defined(__clang__)
#pragma unroll
#endif
    for (int s = r; s < nk; ++s) { acc[k] += B[r] * B[s] + B[nk + r] * B[nk + s]; ++k; }
  }
#if defined(__clang__)
#pragma unroll
#endif
  for (int r = 0; r < nk; ++r) acc[nh + r] += B[r] * d[0] + B[nk + r] * d[1];
  acc[nh + nk] += d[0] * d[0] + d[1] * d[1];
  return true;
}
// One sample of a cost sweep, through the comparer's own cmp_diff_sample at the identity rotation (p.model_b, p.Kb and p.pre_b hold the
// target): the map vc_comparer gives for A against the result holds the very same d.  false: left out.
VC_HD bool cvt_cost_sample(const CmpPlan& p, const double* a, double qx, double qy, double* sq) {
  const double I[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
  double d[2];
  if (!cmp_diff_sample(p, I, a, qx, qy, d)) return false;
  *sq = cmp_norm2(d[0], d[1]);
  return true;
}

// ---- host side --------------------------------------------------------------------------------------------------------------------
inline bool cvt_model_ok(int m) { return m >= 0 && m <= kRational6; }
// the arguments of a run: a radius above 0, a finite start (or none), no mask bit at or above nk
inline bool cvt_run_args_ok(int model_b, double fit_radius, const double* start, unsigned free_mask) {
  const int nk = model_nk(model_b);
  if (!(fit_radius > 0.0) || !(fit_radius <= 1e300)) return false;
  if (free_mask >> nk) return false;
  if (start) for (int k = 0; k < nk; ++k) if (!(fabs(start[k]) <= 1e300)) return false;
  return true;
}
// the start without a caller's: [fu fv u0 v0] of A, distortion 0 (fov: w = kCvtFovStart)
inline void cvt_default_start(int model_b, const double* Ka, double* K) {
  for (int k = 0; k < 10; ++k) K[k] = k < 4 ? Ka[k] : 0.0;
  if (model_b == kFov) K[4] = kCvtFovStart;
}

struct CvtFit {
  double K[10];
  int status, iterations;        // iterations: trial points evaluated
  long long n_fit, n_left_out;
  double cost0, cost;            // E / 2 at the start and at K: the loop's own sums (the callers report those of values-only sweeps instead)
};

// (H + D) delta = -g on the N free parameters; M = H + D on entry (full, row-major), delta = -g.  false: no factorisation.
template <int N>
inline bool cvt_solve_n(double* M, double* delta) {
  if (!chol_small<N>(M)) return false;
  fwd_solve<N>(M, delta); bwd_solve<N>(M, delta);
  return true;
}
inline bool cvt_solve(int n, double* M, double* delta) {
  switch (n) {
    case 1: return cvt_solve_n<1>(M, delta); case 2: return cvt_solve_n<2>(M, delta); case 3: return cvt_solve_n<3>(M, delta);
    case 4: return cvt_solve_n<4>(M, delta); case 5: return cvt_solve_n<5>(M, delta); case 6: return cvt_solve_n<6>(M, delta);
    case 7: return cvt_solve_n<7>(M, delta); case 8: return cvt_solve_n<8>(M, delta); case 9: return cvt_solve_n<9>(M, delta);
    case 10: return cvt_solve_n<10>(M, delta);
  }
  return false;
}

// Levenberg-Marquardt on E(K_b) from `start` with the rules of LmRules.  eval(K, sums) fills the cvt_nsums(nk) sums of one linearisation at K
// and returns 0, or a status that ends the fit and is handed on.  free_mask: bit k set = K[k] is free, 0 = all; a fixed parameter keeps its
// start value -- its rows and columns are dropped from the summed system here, the sweep does not know about it.
//   cost = E / 2; (H + D) delta = -g with D = lm_clamped_diag(diag H, 1) / radius; model_change = -g.delta / 2 + delta^T D delta / 2.
//   No factorisation or model_change <= 0: radius *= kInvalidShrink, kMaxInvalid in a row end the fit as failed.
//   |delta| <= kCvtStepTol (|x_free| + kCvtStepTol): converged, the step is not taken.
//   Accepted when (cost - trial) / model_change > kMinRelativeDecrease: the radius grows by the quality and the decrease factor resets; then
//   |cost change| <= kCvtCostTol cost (the cost before the step): converged.  Rejected, a non-finite trial included: radius /= factor, the
//   factor doubles; a radius below kMinRadius ends the fit as failed.  max_iters trials (<= 0: 50, above 200: 200) end it with status 1.
// Returns 0, -1 (2 n_fit below the number of free parameters, or a first evaluation that is not finite) or eval's status.
template <class Eval>
inline int cvt_levenberg_marquardt(Eval&& eval, int nk, const double* start, unsigned free_mask, int max_iters, long long n_fit, CvtFit* f) {
  const int cap = max_iters <= 0 ? kCvtDefaultIters : max_iters > kCvtMaxIters ? kCvtMaxIters : max_iters;
  const int nh = cvt_nh(nk);
  int idx[10], nf = 0;
  for (int k = 0; k < nk; ++k) if (free_mask == 0 || ((free_mask >> k) & 1)) idx[nf++] = k;
  double cur[kCvtMaxSums], trial[kCvtMaxSums], xt[10];
  for (int k = 0; k < 10; ++k) f->K[k] = k < nk ? start[k] : 0.0;
  f->status = kCvtMaxItersReached; f->iterations = 0; f->n_fit = n_fit; f->n_left_out = 0; f->cost0 = f->cost = 0.0;
  if (2 * n_fit < (long long)nf) return -1;
  int rc = eval(f->K, cur);
  if (rc != 0) return rc;
  double cost = 0.5 * cur[nh + nk];
  if (!(fabs(cost) <= 1e300)) return -1;
  f->cost0 = cost;
  double radius = LmRules::kInitialRadius, decrease = LmRules::kInitialDecrease;
  int invalid = 0;
  while (f->iterations < cap) {
    // ---- the free block of the summed system ----------------------------------------------------------------------------------
    double M[100], D[10], g[10], delta[10];
    for (int a = 0; a < nf; ++a) {
      for (int b = a; b < nf; ++b) {
        const int r = idx[a], s = idx[b];                      // r <= s: packed index of (r, s)
        const double h = cur[r * nk - (r * (r - 1)) / 2 + (s - r)];
        M[a * nf + b] = h; M[b * nf + a] = h;
      }
      g[a] = cur[nh + idx[a]];
    }
    const double ir = 1.0 / radius;
    for (int a = 0; a < nf; ++a) { D[a] = lm_clamped_diag(M[a * nf + a], 1.0) * ir; M[a * nf + a] += D[a]; delta[a] = -g[a]; }
    const bool ok = cvt_solve(nf, M, delta);
    double model_change = 0.0, step2 = 0.0, x2 = 0.0;
    if (ok) {
      double gd = 0.0, dld = 0.0;
      for (int a = 0; a < nf; ++a) { gd += g[a] * delta[a]; dld += delta[a] * D[a] * delta[a]; step2 += delta[a] * delta[a]; x2 += f->K[idx[a]] * f->K[idx[a]]; }
      model_change = -0.5 * gd + 0.5 * dld;
    }
    if (!ok || !(model_change > 0.0)) {                        // (NaN fails the comparison too)
      if (++invalid >= LmRules::kMaxInvalid) { f->status = kCvtFailed; break; }
      radius *= LmRules::kInvalidShrink;
      continue;
    }
    invalid = 0;
    if (sqrt(step2) <= kCvtStepTol * (sqrt(x2) + kCvtStepTol)) { f->status = kCvtConverged; break; }
    // ---- the trial point -------------------------------------------------------------------------------------------------------
    for (int k = 0; k < 10; ++k) xt[k] = f->K[k];
    for (int a = 0; a < nf; ++a) xt[idx[a]] += delta[a];
    ++f->iterations;
    if ((rc = eval(xt, trial)) != 0) return rc;
    const double cost_t = 0.5 * trial[nh + nk];
    const bool finite = fabs(cost_t) <= 1e300;
    const double change = cost - cost_t, quality = change / model_change;
    if (finite && quality > LmRules::kMinRelativeDecrease) {
      for (int k = 0; k < 10; ++k) f->K[k] = xt[k];
      for (int k = 0; k < nh + nk + 3; ++k) cur[k] = trial[k];
      const double q = 2.0 * quality - 1.0;
      radius = fmin(LmRules::kMaxRadius, radius / fmax(1.0 / 3.0, 1.0 - q * q * q));
      decrease = LmRules::kInitialDecrease;
      const double before = cost;
      cost = cost_t;
      if (fabs(change) <= kCvtCostTol * before) { f->status = kCvtConverged; break; }
    } else {                                                   // rejected (a non-finite trial cost included): more damping
      radius = radius / decrease; decrease *= 2.0;
      if (radius < LmRules::kMinRadius) { f->status = kCvtFailed; break; }
    }
  }
  f->cost = cost;
  f->n_left_out = (long long)cur[nh + nk + 2];
  return 0;
}

}  // namespace vc
