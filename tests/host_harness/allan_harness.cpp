// TEST INFRASTRUCTURE: the arithmetic of the IMU noise characterisation (vicalib_amd/csrc/vc_allan.hpp, VC_HD) compiled for the host, so that the
// CPU suite can hold it against tests/allan_ref.py without a GPU.  The second difference, the term, the divisor, the quiet test, the longest
// run, the factors and the fit are the very functions the kernels and the library run; what the kernels add is the order of the sums, which
// are plain loops in sample order here.  allan_harness_gyro_variance propagates a block of the visual-inertial solve's IMU weights
// (vc_imu_weights.hpp) with gyro noise alone: the check behind "sigma = N / sqrt(tau0)" (DESIGN 4.18).
// With -DALLAN_HARNESS_MAIN the file is a program of its own that runs every entry point once on a small log (the sanitizer build).
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>
#include "../../vicalib_amd/csrc/vc_imu_weights.hpp"
#include "../../vicalib_amd/csrc/vc_allan.hpp"

extern "C" {

// the scan's block size, the sweep's chunk length, the largest log, the first n that needs a second tile of block totals
void allan_harness_constants(int out[4]) {
  out[0] = vc::kAllanScanBlock; out[1] = vc::kAllanChunk; out[2] = vc::kAllanMaxN; out[3] = vc::kAllanScanBlock * vc::kAllanScanBlock + 1;
}

// gyro, accel: n x 3 -> means[6], S: 6 x (n + 1), channel-major
void allan_harness_prefix(int n, const double* gyro, const double* accel, double* means, double* S) {
  for (int c = 0; c < 6; ++c) {
    const double* src = c < 3 ? gyro + c : accel + (c - 3);
    double sum = 0.0;
    for (int i = 0; i < n; ++i) sum += src[3 * (size_t)i];
    means[c] = sum / (double)n;
    double* s = S + (size_t)c * ((size_t)n + 1);
    s[0] = 0.0;
    for (int i = 0; i < n; ++i) s[i + 1] = s[i] + (src[3 * (size_t)i] - means[c]);
  }
}

// avar: 6 x n_m over the samples [first, first + count); returns 1 for a factor outside 1 .. count / 2
int allan_harness_avar(int n, const double* S, int first, int count, int n_m, const int* m, double* avar, int* terms) {
  for (int j = 0; j < n_m; ++j)
    if (m[j] < 1 || m[j] > count / 2) return 1;
  for (int c = 0; c < 6; ++c) {
    const double* s = S + (size_t)c * ((size_t)n + 1) + first;
    for (int j = 0; j < n_m; ++j) {
      const int t = vc::allan_terms(count, m[j]);
      double sum = 0.0;
      for (int k = 0; k < t; ++k) sum += vc::allan_term(s, k, m[j]);
      avar[(size_t)c * n_m + j] = vc::allan_avar(sum, m[j], t);
      if (terms) terms[j] = t;
    }
  }
  return 0;
}

// the static stretch: range[2] = first, count; returns 1 (range untouched) when no start is quiet
int allan_harness_static(int n, const double* S, int window, double gyro_thr, double accel_thr, int* range, int* n_quiet) {
  const int n_starts = n - 2 * window + 1;
  std::vector<unsigned char> mask((size_t)n_starts);
  for (int k = 0; k < n_starts; ++k) mask[k] = vc::allan_quiet(S, (size_t)n + 1, k, window, gyro_thr, accel_thr) ? 1 : 0;
  int k0 = 0, k1 = 0;
  if (!vc::allan_longest_run(mask.data(), n_starts, &k0, &k1, n_quiet)) return 1;
  range[0] = k0; range[1] = k1 + 2 * window - k0;
  return 0;
}
// the statistic of one window start for both sensors
void allan_harness_window_change(int n, const double* S, int window, int k, double out[2]) {
  out[0] = vc::allan_window_change(S, (size_t)n + 1, 0, k, window); out[1] = vc::allan_window_change(S, (size_t)n + 1, 1, k, window);
}

int allan_harness_factors(int n_used, int per_decade, double max_fraction, int cap, int* m, double* rel_err) {
  return vc::allan_factors(n_used, per_decade, max_fraction, cap, m, rel_err);
}

int allan_harness_fit(int n, const double* tau, const double* avar, const double* rel_err, double out[5], int* mask) {
  const vc::AllanFit f = vc::allan_fit(n, tau, avar, rel_err);
  out[0] = f.N; out[1] = f.B; out[2] = f.K; out[3] = f.rms_log; out[4] = (double)f.n_points;
  *mask = f.mask;
  return f.status;
}

// A block of T seconds at step dt, the device at rest with the identity attitude, gyro noise sigma alone, through the maps and the noise
// term the solve's weights use: out[0] = the variance of the rotation about x at the block's end (4 x the variance of q_x: q = [theta / 2, 1]
// to first order), out[1] = sigma^2 dt T, out[2] = the same variance at step dt / 2 and the same T.
static double gyro_variance(double sigma, double dt, double T) {
  using namespace vc;
  const int n_int = (int)std::floor(T / dt + 0.5);
  Meas<double> z0, z1;
  for (int i = 0; i < 3; ++i) { z0.w[i] = z1.w[i] = 0.0; z0.a[i] = z1.a[i] = 0.0; }
  z0.time = 0.0; z1.time = dt;
  const double q[4] = {0.0, 0.0, 0.0, 1.0}, b[6] = {0, 0, 0, 0, 0, 0}, sf[6] = {1, 1, 1, 1, 1, 1};
  double f[kWMapF], g[kWMapG], P[kWMapF], Pn[kWMapF], Sp[kWMapQ], term[kWMapQ];
  w_interval_maps(q, z0, z1, b, sf, f, g);
  for (int e = 0; e < kWMapQ; ++e) Sp[e] = 0.0;
  w_map_identity(P);
  for (int m = n_int; m >= 1; --m) {
    w_noise_term(P, g, sigma * sigma, 0.0, term);
    for (int e = 0; e < kWMapQ; ++e) Sp[e] += term[e];
    w_map_compose(P, f, Pn);
    for (int e = 0; e < kWMapF; ++e) P[e] = Pn[e];
  }
  return 4.0 * Sp[w_qidx(3, 3)];
}
void allan_harness_gyro_variance(double sigma, double dt, double T, double out[3]) {
  out[0] = gyro_variance(sigma, dt, T);
  out[1] = sigma * sigma * dt * T;
  out[2] = gyro_variance(sigma, 0.5 * dt, T);
}

}  // extern "C"

#ifdef ALLAN_HARNESS_MAIN
int main() {
  const int n = 3 * vc::kAllanScanBlock + 7;
  std::vector<double> gyro(3 * (size_t)n), accel(3 * (size_t)n), S(6 * ((size_t)n + 1));
  unsigned long long x = 88172645463325252ull;
  auto rnd = [&]() { x ^= x << 13; x ^= x >> 7; x ^= x << 17; return (double)(x >> 11) / 9007199254740992.0 - 0.5; };
  for (int i = 0; i < n; ++i)
    for (int c = 0; c < 3; ++c) {
      const bool moving = i >= 300 && i < 340;
      gyro[3 * (size_t)i + c] = 2e-3 * rnd() + (moving ? 0.5 * rnd() : 0.0);
      accel[3 * (size_t)i + c] = 2e-2 * rnd() + (c == 2 ? 9.81 : 0.0) + (moving ? 2.0 * rnd() : 0.0);
    }
  double means[6];
  allan_harness_prefix(n, gyro.data(), accel.data(), means, S.data());
  int range[2] = {0, n}, n_quiet = 0;
  const int st = allan_harness_static(n, S.data(), 10, 0.02, 0.2, range, &n_quiet);
  std::vector<int> m(64);
  std::vector<double> e(64);
  const int n_m = allan_harness_factors(range[1], 10, 1.0 / 9.0, 64, m.data(), e.data());
  std::vector<double> avar(6 * (size_t)n_m), tau(n_m);
  std::vector<int> terms(n_m);
  const int rc = allan_harness_avar(n, S.data(), range[0], range[1], n_m, m.data(), avar.data(), terms.data());
  for (int j = 0; j < n_m; ++j) tau[j] = 0.005 * m[j];
  double fit[5], var[3];
  int mask = 0;
  const int fs = allan_harness_fit(n_m, tau.data(), avar.data(), e.data(), fit, &mask);
  allan_harness_gyro_variance(1e-3, 0.005, 0.5, var);
  std::printf("static %d: [%d, +%d), %d quiet starts; %d factors (rc %d), adev(gx, m=1) %.6e; fit status %d mask %d N %.6e; rotation variance %.6e against %.6e\n",
              st, range[0], range[1], n_quiet, n_m, rc, std::sqrt(avar[0]), fs, mask, fit[0], var[0], var[1]);
  return (st == 0 && rc == 0 && n_m > 0) ? 0 : 1;
}
#endif
