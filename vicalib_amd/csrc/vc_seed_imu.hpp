// vc_seed_imu.hpp -- the arithmetic of the inertial seed (vc_seed_imu.hip): the rotation camera <- IMU of camera 0, the time offset between
// the two clocks, the gyro bias and the direction of gravity, in closed form from the PnP rotations of the frames and the IMU log, before
// anything is solved.  VC_HD: the kernels and tests/host_harness/seed_imu_harness.cpp run the same functions; what the kernels add is the
// order of the sums.  Everything is fp64.
//
// Conventions (vc_imu.hpp imu_range; vicalib_amd/synth.py): a sample stamped t was taken at image-clock time t + offset; T_wk = T_wc T_ck,
// so R_wc^T = R_ck R_wk^T; the camera-frame rate is w_c = R_ck (z_g + b_g) with the scale factors taken as 1.
//   prefix integrals of the piecewise-linear signal, six channels:  G_0 = 0, G_k = G_{k-1} + 0.5 (y_{k-1} + y_k)(t_k - t_{k-1})
//   G(tau), t_k <= tau <= t_{k+1}:  G_k + s (y_k + 0.5 (y_{k+1} - y_k) s / h),  s = tau - t_k, h = t_{k+1} - t_k      (exact for the interpolant)
//   camera rate of interval i (frames i, i + 1):  a_i = log(R_wc,i^T R_wc,i+1) / (t_{i+1} - t_i)
//   IMU rate at lag d:                            b_i(d) = (G(t_{i+1} - d) - G(t_i - d)) / (t_{i+1} - t_i)
// Per lag, over the intervals valid at that lag, 18 moments: n, sum a', sum b, sum |a'|^2, sum |b|^2, sum b a'^T, with a' = a - a_p the rate
// relative to the pivot a_p, the rate of the first valid interval (a constant rate then centres to rounding of the DIFFERENCES, not of the
// squares).  Centred: H = sum (b - bm)(a - am)^T; R_ck = rigid_rotation(H) (Horn, vc_rectify.hpp: takes the first bundle onto the second);
// J = (Sa + Sb - 2 tr(R H)) / n; b_g = R^T am - bm.
#pragma once
#include <cmath>
#include <cstddef>
#include <algorithm>
#include <limits>
#include <vector>
#include "vc_rectify.hpp"

namespace vc {

constexpr int kSeedImuChannels = 6;        // gx gy gz ax ay az, channel-major
constexpr int kSeedImuMaxN = 1 << 24;      // samples of a log
constexpr int kSeedImuScanBlock = 256;     // samples per block of the prefix integrals: one per thread; the totals are scanned in tiles of as many
constexpr int kSeedImuChunk = 1024;        // intervals of one lag's sums per workgroup of the sweep: a constant, not the device's CU count
constexpr int kSeedImuSearchSteps = 25;    // bisections that find a sample interval among 2^24 + 1 candidates
constexpr int kSeedImuMoments = 18;        // n, sum a' (3), sum b (3), sum |a'|^2, sum |b|^2, sum b a'^T (9, row-major: b's component is the row)
constexpr int kSeedImuMaxLags = 65535;     // lags of one launch (a grid dimension); the host runs longer lists in pieces
constexpr int kSeedImuMaxLattice = 1 << 20;

enum { kSeedImuOk = 0, kSeedImuTooFew = 1, kSeedImuEdge = 2, kSeedImuNotFinite = 3 };

struct SimuLog {
  int n, steps;                 // samples; bisections: simu_search_steps(n)
  const double* t;              // n
  const double* y;              // 6 x n
  const double* G;              // 6 x n
};

VC_HD int simu_chunks(int n_int) { return (n_int + kSeedImuChunk - 1) / kSeedImuChunk; }
VC_HD int simu_min_valid(int min_intervals) { return min_intervals > 3 ? min_intervals : 3; }
VC_HD int simu_search_steps(int n) { int s = 0; while (s < kSeedImuSearchSteps && (1 << s) < n + 1) ++s; return s; }
VC_HD double simu_prefix_inc(double y0, double y1, double t0, double t1) { return 0.5 * (y0 + y1) * (t1 - t0); }

// upper_bound(t, tau) - 1, clamped to 0 .. n - 2: the sample interval that holds tau (the last one for tau = t_{n-1})
VC_HD int simu_interval_of(const SimuLog& L, double tau) {
  int lo = 0, hi = L.n;
  for (int s = 0; s < L.steps; ++s) {
    if (lo < hi) {                                        // (lo < hi: mid <= n - 1)
      const int mid = (lo + hi) >> 1;
      if (L.t[mid] <= tau) lo = mid + 1; else hi = mid;
    }
  }
  int k = lo - 1;
  k = k < 0 ? 0 : k;
  return k > L.n - 2 ? L.n - 2 : k;
}
VC_HD double simu_G_at(const SimuLog& L, int c, int k, double tau) {
  const double* y = L.y + (size_t)c * L.n;
  const double s = tau - L.t[k], h = L.t[k + 1] - L.t[k];
  return L.G[(size_t)c * L.n + k] + s * (y[k] + 0.5 * (y[k + 1] - y[k]) * s / h);
}
// the mean of channels c0 .. c0 + 2 over [tau0, tau1] (inv_dt = 1 / (tau1 - tau0)); false when the stretch leaves the log
VC_HD bool simu_mean3(const SimuLog& L, int c0, double tau0, double tau1, double inv_dt, double* out) {
  if (!(tau0 >= L.t[0]) || !(tau1 <= L.t[L.n - 1])) return false;
  const int k0 = simu_interval_of(L, tau0), k1 = simu_interval_of(L, tau1);
#pragma unroll
  for (int c = 0; c < 3; ++c) out[c] = (simu_G_at(L, c0 + c, k1, tau1) - simu_G_at(L, c0 + c, k0, tau0)) * inv_dt;
  return true;
}

// a_i and 1 / dt of the interval between two frames; false: a frame without a seed, or 0 < dt <= max_gap_s does not hold
VC_HD bool simu_cam_rate(const double* q0, const double* q1, bool ok0, bool ok1, double t0, double t1, double max_gap_s, double* a, double* inv_dt) {
  const double dt = t1 - t0;
  a[0] = a[1] = a[2] = 0.0; *inv_dt = 0.0;
  if (!ok0 || !ok1 || !(dt > 0.0) || !(dt <= max_gap_s)) return false;
  const double c0[4] = {-q0[0], -q0[1], -q0[2], q0[3]};
  double q[4];
  quat_mul(c0, q1, q);                                      // R_wc,i^T R_wc,i+1 (any positive scale: the angle is a ratio)
  const double sg = q[3] < 0.0 ? -1.0 : 1.0;
  const double nv = sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2]), w = sg * q[3];
  const double k = nv > 1e-12 * w ? 2.0 * atan2(nv, w) / nv : 2.0 / w;
  *inv_dt = 1.0 / dt;
  for (int c = 0; c < 3; ++c) a[c] = sg * q[c] * k * *inv_dt;
  return true;
}

// x + y + z in an order that does not depend on the order of the arguments: smallest, middle, largest
VC_HD double simu_sum3_sym(double x, double y, double z) {
  const double lo = fmin(x, fmin(y, z)), hi = fmax(x, fmax(y, z));
  const double mid = fmax(fmin(x, y), fmin(fmax(x, y), z));
  return (lo + mid) + hi;
}
// one interval's 18 terms, added to m
VC_HD void simu_accumulate(const double* a_rel, const double* b, double* m) {
  m[0] += 1.0;
#pragma unroll
  for (int c = 0; c < 3; ++c) { m[1 + c] += a_rel[c]; m[4 + c] += b[c]; }
  m[7] += (a_rel[0] * a_rel[0] + a_rel[1] * a_rel[1]) + a_rel[2] * a_rel[2];
  m[8] += simu_sum3_sym(b[0] * b[0], b[1] * b[1], b[2] * b[2]);
#pragma unroll
  for (int r = 0; r < 3; ++r)
#pragma unroll
    for (int c = 0; c < 3; ++c) m[9 + 3 * r + c] += b[r] * a_rel[c];
}
// the centred sum |a - am|^2 of a lag's moments
VC_HD double simu_Sa(const double* m) {
  return m[7] - ((m[1] * m[1] + m[2] * m[2]) + m[3] * m[3]) / m[0];
}

// One lag from its moments.  Horn's fit runs on the gyro channels in a canonical cyclic order -- the channel whose row of H is the longest
// first (the lowest index among equals) -- and the columns of R go back to the caller's order: the three channels permuted cyclically give
// the same J bits and the same R with its columns permuted.  Fewer than min_valid intervals: J = +inf, R = I, bias = 0.
VC_HD void simu_fit(const double* m, const double* pivot, int min_valid, double* J, double* R, double* bias, int* count) {
  const double n = m[0];
  *count = (int)n;
  if (*count < min_valid) {
    *J = INFINITY;
    for (int k = 0; k < 9; ++k) R[k] = (k % 4 == 0) ? 1.0 : 0.0;
    bias[0] = bias[1] = bias[2] = 0.0;
    return;
  }
  const double in = 1.0 / n;
  const double am[3] = {m[1] * in, m[2] * in, m[3] * in}, bm[3] = {m[4] * in, m[5] * in, m[6] * in};
  const double Sa = simu_Sa(m);
  const double Sb = m[8] - n * simu_sum3_sym(bm[0] * bm[0], bm[1] * bm[1], bm[2] * bm[2]);
  double H[9], key[3];
#pragma unroll
  for (int r = 0; r < 3; ++r) {
#pragma unroll
    for (int c = 0; c < 3; ++c) H[3 * r + c] = m[9 + 3 * r + c] - n * bm[r] * am[c];
    key[r] = fma(H[3 * r + 2], H[3 * r + 2], fma(H[3 * r + 1], H[3 * r + 1], H[3 * r] * H[3 * r]));      // (fma spelled out: see the bias below)
  }
  const int s = (key[0] >= key[1] && key[0] >= key[2]) ? 0 : (key[1] >= key[2] ? 1 : 2);
  double Hc[9], Rc[9];                                       // rows s, s + 1, s + 2 (cyclic), by selects: no run-time index
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const double h0 = H[c], h1 = H[3 + c], h2 = H[6 + c];
    Hc[c] = s == 0 ? h0 : (s == 1 ? h1 : h2);
    Hc[3 + c] = s == 0 ? h1 : (s == 1 ? h2 : h0);
    Hc[6 + c] = s == 0 ? h2 : (s == 1 ? h0 : h1);
  }
  rigid_rotation(Hc, Rc);
  double tr = 0.0;
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) tr += Rc[3 * i + j] * Hc[3 * j + i];
  *J = ((Sa + Sb) - 2.0 * tr) * in;
#pragma unroll
  for (int r = 0; r < 3; ++r) {                              // column j of Rc is column (s + j) mod 3 of R
    const double c0 = Rc[3 * r], c1 = Rc[3 * r + 1], c2 = Rc[3 * r + 2];
    R[3 * r] = s == 0 ? c0 : (s == 1 ? c2 : c1);
    R[3 * r + 1] = s == 0 ? c1 : (s == 1 ? c0 : c2);
    R[3 * r + 2] = s == 0 ? c2 : (s == 1 ? c1 : c0);
  }
  const double a_full[3] = {pivot[0] + am[0], pivot[1] + am[1], pivot[2] + am[2]};
#pragma unroll
  // (the fused multiply-adds are spelled out: left to the compiler, which product of x y + z w it fuses may differ from one component to
  //  the next, and a permuted channel would not get the bits of the channel it came from)
  for (int c = 0; c < 3; ++c) bias[c] = fma(R[6 + c], a_full[2], fma(R[3 + c], a_full[1], R[c] * a_full[0])) - bm[c];
}

// one interval's term of the gravity sum: R_wc,i R_ck abar_i
VC_HD void simu_gravity_term(const double* q_wc, const double* R_ck, const double* abar, double* out) {
  double v[3];
  for (int r = 0; r < 3; ++r) v[r] = (R_ck[3 * r] * abar[0] + R_ck[3 * r + 1] * abar[1]) + R_ck[3 * r + 2] * abar[2];
  const double nq = 1.0 / sqrt((q_wc[0] * q_wc[0] + q_wc[1] * q_wc[1]) + (q_wc[2] * q_wc[2] + q_wc[3] * q_wc[3]));
  const double q[4] = {q_wc[0] * nq, q_wc[1] * nq, q_wc[2] * nq, q_wc[3] * nq};
  quat_rotate(q, v, out);
}

// ---- host only -----------------------------------------------------------------------------------------------------------------------
struct SeedImuData {
  int n_frames; const double* frame_t; const double* frame_q; const unsigned char* frame_ok;
  int n_samples; const double* imu_t; const double* gyro; const double* accel;
  double max_gap_s; int min_intervals;
};
// what vc_seed_imu_sweep refuses with VC_ERR_BAD_ARG (n_samples above kSeedImuMaxN is the caller's to refuse first, as unsupported)
inline bool simu_data_ok(const SeedImuData& d) {
  if (!d.frame_t || !d.frame_q || !d.frame_ok || !d.imu_t || !d.gyro || !d.accel) return false;
  if (d.n_frames < 2 || d.n_samples < 2 || !(d.max_gap_s > 0.0) || d.min_intervals < 1) return false;
  for (int i = 0; i < d.n_frames; ++i) {
    if (!std::isfinite(d.frame_t[i]) || (i > 0 && !(d.frame_t[i] > d.frame_t[i - 1]))) return false;
    if (d.frame_ok[i]) {
      const double* q = d.frame_q + 4 * (size_t)i;
      const double nq = std::sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
      if (!(nq >= 0.5 && nq <= 2.0)) return false;
    }
  }
  for (int k = 0; k < d.n_samples; ++k) {
    if (!std::isfinite(d.imu_t[k]) || (k > 0 && !(d.imu_t[k] > d.imu_t[k - 1]))) return false;
    for (int c = 0; c < 3; ++c)
      if (!std::isfinite(d.gyro[3 * (size_t)k + c]) || !std::isfinite(d.accel[3 * (size_t)k + c])) return false;
  }
  return true;
}
inline bool simu_lags_ok(int n_lags, const double* lags) {
  if (n_lags < 1 || !lags) return false;
  for (int j = 0; j < n_lags; ++j) if (!std::isfinite(lags[j])) return false;
  return true;
}
// the first interval with a camera rate (frames ok, gap in range), -1 without one: its rate is the pivot
inline int simu_pivot_interval(const SeedImuData& d) {
  for (int i = 0; i + 1 < d.n_frames; ++i) {
    const double dt = d.frame_t[i + 1] - d.frame_t[i];
    if (d.frame_ok[i] && d.frame_ok[i + 1] && dt > 0.0 && dt <= d.max_gap_s) return i;
  }
  return -1;
}
// the median interval between samples (the upper one of an even number)
inline double simu_median_step(int n, const double* t) {
  std::vector<double> dt((size_t)n - 1);
  for (int k = 0; k + 1 < n; ++k) dt[k] = t[k + 1] - t[k];
  std::nth_element(dt.begin(), dt.begin() + dt.size() / 2, dt.end());
  return dt[dt.size() / 2];
}
// the lowest value's index, the lowest index among equals; -1 when nothing is finite
inline int simu_argmin(const std::vector<double>& J) {
  int best = -1;
  for (size_t j = 0; j < J.size(); ++j)
    if (std::isfinite(J[j]) && (best < 0 || J[j] < J[(size_t)best])) best = (int)j;
  return best;
}

struct SeedImuResult {
  int status = kSeedImuTooFew, count = 0, coarse_index = -1, n_coarse = 0;
  double time_offset = 0.0, R_ck[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1}, gyro_bias[3] = {0, 0, 0}, g_dir[2] = {0, 0}, rms = 0.0, signal = 0.0, step = 0.0;
  std::vector<double> coarse_lags, coarse_J;
};

// The pick.  A backend evaluates lags: sweep(n, lags, J, R, bias, count, moments) and gravity(lag, R_ck, u[3]) -- the kernels in the library,
// plain loops in the host harness; both return a status of the C ABI (0 = ok), handed on.
//  1. the coarse lattice -range_s .. +range_s at step_s (<= 0: the median sample interval); the lowest J, the lowest index among equals;
//     a minimum on either end: status 2, nothing else filled; no lag with max(3, min_intervals) intervals: status 1
//  2. a fine lattice of 4 fine + 1 lags at step / fine centred on it; a parabola through the three points around its minimum (the minimum
//     itself when it sits on an edge, or when the three points do not curve upwards)
//  3. one more lag at the refined d: R_ck, b_g, rms = sqrt(J), signal = sqrt(Sa / n); gravity there
template <class Backend>
inline int simu_pick(Backend& be, const SeedImuData& d, double range_s, double step_s, int fine, SeedImuResult* r) {
  *r = SeedImuResult();
  const double step = step_s > 0.0 ? step_s : simu_median_step(d.n_samples, d.imu_t);
  r->step = step;
  const double sides = std::floor(range_s / step + 1e-9);
  if (!(sides < 0.5 * kSeedImuMaxLattice)) return -2;                                   // VC_ERR_BAD_ARG: the lattice has too many lags
  const int n_side = sides >= 1.0 ? (int)sides : 1, n_coarse = 2 * n_side + 1;
  r->n_coarse = n_coarse;
  r->coarse_lags.resize((size_t)n_coarse); r->coarse_J.resize((size_t)n_coarse);
  for (int j = 0; j < n_coarse; ++j) r->coarse_lags[(size_t)j] = (double)(j - n_side) * step;
  std::vector<int> count((size_t)n_coarse);
  int rc = be.sweep(n_coarse, r->coarse_lags.data(), r->coarse_J.data(), nullptr, nullptr, count.data(), nullptr);
  if (rc != 0) return rc;
  const int jc = simu_argmin(r->coarse_J);
  r->coarse_index = jc;
  if (jc < 0) {
    bool inf_only = true;
    for (int j = 0; j < n_coarse; ++j) inf_only = inf_only && r->coarse_J[(size_t)j] == std::numeric_limits<double>::infinity();
    r->status = inf_only ? kSeedImuTooFew : kSeedImuNotFinite;
    return 0;
  }
  if (jc == 0 || jc == n_coarse - 1) { r->status = kSeedImuEdge; return 0; }
  const int n_fine = 4 * fine + 1;
  const double h = step / (double)fine;
  std::vector<double> fl((size_t)n_fine), fJ((size_t)n_fine);
  for (int k = 0; k < n_fine; ++k) fl[(size_t)k] = r->coarse_lags[(size_t)jc] + (double)(k - 2 * fine) * h;
  rc = be.sweep(n_fine, fl.data(), fJ.data(), nullptr, nullptr, nullptr, nullptr);
  if (rc != 0) return rc;
  const int jf = simu_argmin(fJ);
  if (jf < 0) { r->status = kSeedImuNotFinite; return 0; }
  double dd = fl[(size_t)jf];
  if (jf > 0 && jf < n_fine - 1) {
    const double jm = fJ[(size_t)jf - 1], j0 = fJ[(size_t)jf], jp = fJ[(size_t)jf + 1], den = (jm - 2.0 * j0) + jp;
    if (std::isfinite(jm) && std::isfinite(jp) && den > 0.0) dd += 0.5 * (jm - jp) / den * h;
  }
  double J = 0.0, mom[kSeedImuMoments], u[3] = {0, 0, 0};
  rc = be.sweep(1, &dd, &J, r->R_ck, r->gyro_bias, &r->count, mom);
  if (rc != 0) return rc;
  r->time_offset = dd;
  if (!std::isfinite(J)) { r->status = J == std::numeric_limits<double>::infinity() ? kSeedImuTooFew : kSeedImuNotFinite; return 0; }
  r->rms = std::sqrt(J > 0.0 ? J : 0.0);
  const double sa = simu_Sa(mom);
  r->signal = std::sqrt((sa > 0.0 ? sa : 0.0) / mom[0]);
  rc = be.gravity(dd, r->R_ck, u);
  if (rc != 0) return rc;
  const double nu = std::sqrt(u[0] * u[0] + u[1] * u[1] + u[2] * u[2]);
  r->g_dir[0] = std::asin(u[1] / nu);
  r->g_dir[1] = std::asin(-(u[0] / nu) / std::cos(r->g_dir[0]));
  bool fin = std::isfinite(r->g_dir[0]) && std::isfinite(r->g_dir[1]) && std::isfinite(r->rms) && std::isfinite(r->signal);
  for (int k = 0; k < 9; ++k) fin = fin && std::isfinite(r->R_ck[k]);
  for (int k = 0; k < 3; ++k) fin = fin && std::isfinite(r->gyro_bias[k]);
  r->status = fin ? kSeedImuOk : kSeedImuNotFinite;
  return 0;
}

}  // namespace vc
