// vc_allan.hpp -- the arithmetic of the IMU noise characterisation (vc_allan.hip): the overlapping Allan variance of a static log from the
// prefix sums of its six channels, the averaging factors with their standard error, the quiet-window test, and the fit of white noise, bias
// instability and rate random walk to a curve.  VC_HD: the kernels and tests/host_harness/allan_harness.cpp run the same functions; what the
// kernels add is the order of the sums.  Everything is fp64.
//
// One channel y_0 .. y_{n-1}: S_0 = 0, S_k = sum_{i<k} (y_i - mean), n + 1 values.  For an averaging factor m over the samples [a, b):
//   avar(m) = sum_{k=a}^{b-2m} (S_{k+2m} - 2 S_{k+m} + S_k)^2 / (2 m^2 terms),   terms = (b - a) - 2m + 1.
// The sample period cancels: with tau = m tau0 the textbook form divides the squares by tau^2 and the sums S by 1 / tau0.
#pragma once
#include <cmath>
#include <cstddef>

#ifndef VC_HD
#if defined(__HIPCC__)
#define VC_HD __host__ __device__ __forceinline__
#else
#define VC_HD inline
#endif
#endif

namespace vc {

constexpr int kAllanChannels = 6;          // gx gy gz ax ay az
constexpr int kAllanMaxN = 1 << 24;        // samples of a log (indices and term counts stay ints)
constexpr int kAllanScanBlock = 256;       // samples per block of the prefix sums: one per thread; the totals are scanned in tiles of as many
constexpr int kAllanChunk = 8192;          // terms of one (factor, channel) sum per workgroup of the sweep: a constant, not the device's CU count
constexpr int kAllanMaxFactors = 65535;    // factors of one run (a grid dimension)

// the second difference of the prefix sums: m times the change of the mean between two adjacent windows of m samples
VC_HD double allan_diff(double s2, double s1, double s0) { return (s2 - 2.0 * s1) + s0; }
VC_HD double allan_term(const double* S, int k, int m) {
  const double d = allan_diff(S[k + 2 * m], S[k + m], S[k]);
  return d * d;
}
VC_HD int allan_terms(int count, int m) { return count - 2 * m + 1; }
VC_HD int allan_chunks(int terms) { return (terms + kAllanChunk - 1) / kAllanChunk; }
VC_HD double allan_avar(double sum, int m, int terms) { return sum / ((2.0 * (double)m * (double)m) * (double)terms); }
// IEEE Std 952: the relative standard error of adev at factor m from n_used samples
VC_HD double allan_rel_err(int n_used, int m) { return 1.0 / std::sqrt(2.0 * ((double)n_used / (double)m - 1.0)); }

// Window start k is quiet when the mean of every sensor changes by less than its threshold to the next window of W samples: the norm over the
// sensor's three axes of d_c = (S_{k+2W} - 2 S_{k+W} + S_k) / W.  S: six channels of n1 = n + 1 values each; a threshold <= 0 switches the test off.
VC_HD double allan_window_change(const double* S, size_t n1, int sensor, int k, int W) {
  double q = 0.0;
  for (int c = 0; c < 3; ++c) {
    const double* s = S + (size_t)(3 * sensor + c) * n1;
    const double d = allan_diff(s[k + 2 * W], s[k + W], s[k]) / (double)W;
    q += d * d;
  }
  return std::sqrt(q);
}
VC_HD bool allan_quiet(const double* S, size_t n1, int k, int W, double gyro_thr, double accel_thr) {
  if (gyro_thr > 0.0 && !(allan_window_change(S, n1, 0, k, W) < gyro_thr)) return false;
  if (accel_thr > 0.0 && !(allan_window_change(S, n1, 1, k, W) < accel_thr)) return false;
  return true;
}

// ---- host only -----------------------------------------------------------------------------------------------------------------------
// The longest run of quiet starts k0 .. k1, the earliest among equals; false when none is quiet.  The stretch covers samples [k0, k1 + 2W).
inline bool allan_longest_run(const unsigned char* mask, int n_starts, int* k0, int* k1, int* n_quiet) {
  int best = 0, best_at = 0, run = 0, quiet = 0;
  for (int k = 0; k < n_starts; ++k) {
    if (mask[k]) { ++run; ++quiet; if (run > best) { best = run; best_at = k - run + 1; } }
    else run = 0;
  }
  *n_quiet = quiet;
  if (best == 0) return false;
  *k0 = best_at; *k1 = best_at + best - 1;
  return true;
}

// round(10^(j / per_decade)), j = 0, 1, ..., made strictly increasing, up to max(1, floor(n_used max_fraction)).  Returns the count; writes
// at most cap entries of m (nullable) and rel_err (nullable).  n_used >= 2, per_decade >= 1, 0 < max_fraction <= 0.5: every m has 2m <= n_used.
inline int allan_factors(int n_used, int per_decade, double max_fraction, int cap, int* m, double* rel_err) {
  const double lim = std::floor((double)n_used * max_fraction);
  const int m_max = lim >= 1.0 ? (int)lim : 1;
  int count = 0, last = 0;
  for (int j = 0;; ++j) {
    const double x = std::floor(std::pow(10.0, (double)j / (double)per_decade) + 0.5);
    if (x > (double)m_max) break;
    const int v = (int)x;
    if (v <= last) continue;
    if (count < cap) { if (m) m[count] = v; if (rel_err) rel_err[count] = allan_rel_err(n_used, v); }
    last = v; ++count;
  }
  return count;
}

// avar(tau) = N^2 / tau + (2 ln 2 / pi) B^2 + K^2 tau / 3, the three coefficients >= 0, weights 1 / (avar_j^2 e_j^2).  The seven non-empty
// subsets of the terms (mask 1 .. 7: bit 0 N, bit 1 B, bit 2 K) are solved by their normal equations (columns scaled to unit diagonal,
// Cholesky); among those whose solution is non-negative the smallest weighted residual wins, the lowest mask among equals.  A point whose
// tau, avar or e is not positive and finite is left out.  Status 1: fewer than three points, the model's terms; 2: no feasible subset.
struct AllanFit { double N = 0.0, B = 0.0, K = 0.0, rms_log = 0.0; int mask = 0, status = 0, n_points = 0; };
constexpr double kAllanBiasFactor = 2.0 * 0.6931471805599453 / 3.141592653589793;      // 2 ln 2 / pi
inline void allan_basis(double tau, double* f) { f[0] = 1.0 / tau; f[1] = kAllanBiasFactor; f[2] = tau / 3.0; }
inline double allan_model(double N, double B, double K, double tau) {
  double f[3]; allan_basis(tau, f);
  return (N * N) * f[0] + (B * B) * f[1] + (K * K) * f[2];
}
inline AllanFit allan_fit(int n, const double* tau, const double* avar, const double* rel_err) {
  AllanFit r;
  double A[3][3] = {{0, 0, 0}, {0, 0, 0}, {0, 0, 0}}, g[3] = {0, 0, 0};
  auto usable = [&](int j) {
    return std::isfinite(tau[j]) && std::isfinite(avar[j]) && std::isfinite(rel_err[j]) && tau[j] > 0.0 && avar[j] > 0.0 && rel_err[j] > 0.0;
  };
  for (int j = 0; j < n; ++j) {
    if (!usable(j)) continue;
    const double sw = 1.0 / (avar[j] * rel_err[j]);      // sqrt of the weight: the rows are f / (avar e), the right side 1 / e
    double f[3]; allan_basis(tau[j], f);
    const double y = avar[j] * sw;
    for (int a = 0; a < 3; ++a) { f[a] *= sw; g[a] += f[a] * y; }
    for (int a = 0; a < 3; ++a) for (int b = 0; b < 3; ++b) A[a][b] += f[a] * f[b];
    ++r.n_points;
  }
  if (r.n_points < 3) { r.status = 1; return r; }
  double best = 0.0, best_x[3] = {0, 0, 0};
  for (int mask = 1; mask < 8; ++mask) {
    int idx[3], d = 0;
    for (int a = 0; a < 3; ++a) if (mask & (1 << a)) idx[d++] = a;
    double s[3], L[3][3], z[3], x[3] = {0, 0, 0};
    bool ok = true;
    for (int a = 0; a < d; ++a) { s[a] = std::sqrt(A[idx[a]][idx[a]]); ok = ok && s[a] > 0.0; }
    if (!ok) continue;
    for (int a = 0; a < d && ok; ++a)
      for (int b = 0; b <= a; ++b) {
        double v = A[idx[a]][idx[b]] / (s[a] * s[b]);
        for (int k = 0; k < b; ++k) v -= L[a][k] * L[b][k];
        if (a == b) { if (!(v > 0.0)) { ok = false; break; } L[a][a] = std::sqrt(v); }
        else L[a][b] = v / L[b][b];
      }
    if (!ok) continue;
    for (int a = 0; a < d; ++a) { double v = g[idx[a]] / s[a]; for (int k = 0; k < a; ++k) v -= L[a][k] * z[k]; z[a] = v / L[a][a]; }
    for (int a = d - 1; a >= 0; --a) { double v = z[a]; for (int k = a + 1; k < d; ++k) v -= L[k][a] * x[idx[k]]; x[idx[a]] = v / L[a][a]; }
    for (int a = 0; a < d; ++a) { x[idx[a]] /= s[a]; ok = ok && std::isfinite(x[idx[a]]) && x[idx[a]] >= 0.0; }
    if (!ok) continue;
    double res = 0.0;                                     // the weighted residual, term by term (y.y - g.x would cancel)
    for (int j = 0; j < n; ++j) {
      if (!usable(j)) continue;
      double f[3]; allan_basis(tau[j], f);
      const double e = ((x[0] * f[0] + x[1] * f[1] + x[2] * f[2]) - avar[j]) / (avar[j] * rel_err[j]);
      res += e * e;
    }
    if (r.mask == 0 || res < best) { best = res; r.mask = mask; for (int a = 0; a < 3; ++a) best_x[a] = x[a]; }
  }
  if (r.mask == 0) { r.status = 2; return r; }
  r.N = std::sqrt(best_x[0]); r.B = std::sqrt(best_x[1]); r.K = std::sqrt(best_x[2]);
  double q = 0.0;
  for (int j = 0; j < n; ++j) {
    if (!usable(j)) continue;
    const double l = std::log(allan_model(r.N, r.B, r.K, tau[j]) / avar[j]);
    q += l * l;
  }
  r.rms_log = std::sqrt(q / r.n_points);
  return r;
}

}  // namespace vc
