// TEST INFRASTRUCTURE: the arithmetic of the inertial seed (vicalib_amd/csrc/vc_seed_imu.hpp, VC_HD) compiled for the host, so that the CPU
// suite can hold it against tests/seed_imu_ref.py without a GPU.  The prefix increment, the bounded bisection, the interpolated integral,
// the camera rate, the 18 terms of an interval, the fit of a lag, the gravity term and the pick are the very functions the kernels and the
// library run; what the kernels add is the order of the sums, which are plain loops in sample and interval order here.
// With -DSEED_IMU_HARNESS_MAIN the file is a program of its own that runs every entry point once on a small problem (the sanitizer build).
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>
#include "../../vicalib_amd/csrc/vc_seed_imu.hpp"

namespace {

// the backend of vc::simu_pick in plain loops
struct HostSimu {
  vc::SeedImuData d;
  std::vector<double> y, G, a, inv_dt;
  std::vector<unsigned char> valid;
  double pivot[3] = {0, 0, 0};
  int n_int = 0, min_valid = 3;

  explicit HostSimu(const vc::SeedImuData& data) : d(data) {
    const size_t N = (size_t)d.n_samples;
    y.resize(6 * N); G.resize(6 * N);
    for (size_t k = 0; k < N; ++k)
      for (int c = 0; c < 3; ++c) { y[(size_t)c * N + k] = d.gyro[3 * k + c]; y[(size_t)(3 + c) * N + k] = d.accel[3 * k + c]; }
    for (int c = 0; c < 6; ++c) {
      double* g = G.data() + (size_t)c * N;
      const double* yc = y.data() + (size_t)c * N;
      g[0] = 0.0;
      for (size_t k = 1; k < N; ++k) g[k] = g[k - 1] + vc::simu_prefix_inc(yc[k - 1], yc[k], d.imu_t[k - 1], d.imu_t[k]);
    }
    n_int = d.n_frames - 1; min_valid = vc::simu_min_valid(d.min_intervals);
    a.resize(3 * (size_t)n_int); inv_dt.resize((size_t)n_int); valid.resize((size_t)n_int);
    for (int i = 0; i < n_int; ++i)
      valid[(size_t)i] = vc::simu_cam_rate(d.frame_q + 4 * (size_t)i, d.frame_q + 4 * (size_t)(i + 1), d.frame_ok[i] != 0, d.frame_ok[i + 1] != 0, d.frame_t[i],
                                           d.frame_t[i + 1], d.max_gap_s, &a[3 * (size_t)i], &inv_dt[(size_t)i]) ? 1 : 0;
    const int p = vc::simu_pivot_interval(d);
    if (p >= 0) for (int c = 0; c < 3; ++c) pivot[c] = a[3 * (size_t)p + c];
  }
  vc::SimuLog log() const { return vc::SimuLog{d.n_samples, vc::simu_search_steps(d.n_samples), d.imu_t, y.data(), G.data()}; }

  int sweep(int n_lags, const double* lags, double* J, double* R, double* bias, int* count, double* mom) {
    const vc::SimuLog L = log();
    for (int j = 0; j < n_lags; ++j) {
      double m[vc::kSeedImuMoments];
      for (double& v : m) v = 0.0;
      for (int i = 0; i < n_int; ++i) {
        double b[3];
        if (!valid[(size_t)i] || !vc::simu_mean3(L, 0, d.frame_t[i] - lags[j], d.frame_t[i + 1] - lags[j], inv_dt[(size_t)i], b)) continue;
        const double ar[3] = {a[3 * (size_t)i] - pivot[0], a[3 * (size_t)i + 1] - pivot[1], a[3 * (size_t)i + 2] - pivot[2]};
        vc::simu_accumulate(ar, b, m);
      }
      double Jj, Rj[9], bj[3];
      int cj;
      vc::simu_fit(m, pivot, min_valid, &Jj, Rj, bj, &cj);
      if (J) J[j] = Jj;
      if (R) std::memcpy(R + 9 * (size_t)j, Rj, sizeof(Rj));
      if (bias) std::memcpy(bias + 3 * (size_t)j, bj, sizeof(bj));
      if (count) count[j] = cj;
      if (mom) std::memcpy(mom + vc::kSeedImuMoments * (size_t)j, m, sizeof(m));
    }
    return 0;
  }
  int gravity(double lag, const double* R_ck, double* u) {
    const vc::SimuLog L = log();
    u[0] = u[1] = u[2] = 0.0;
    for (int i = 0; i < n_int; ++i) {
      double abar[3], g[3];
      if (!valid[(size_t)i] || !vc::simu_mean3(L, 3, d.frame_t[i] - lag, d.frame_t[i + 1] - lag, inv_dt[(size_t)i], abar)) continue;
      vc::simu_gravity_term(d.frame_q + 4 * (size_t)i, R_ck, abar, g);
      for (int k = 0; k < 3; ++k) u[k] += g[k];
    }
    return 0;
  }
};

}  // namespace

extern "C" {

// the scan's block size, the sweep's chunk length, the largest log, the bisections, the moments, the lags of one launch
void seed_imu_harness_constants(int out[6]) {
  out[0] = vc::kSeedImuScanBlock; out[1] = vc::kSeedImuChunk; out[2] = vc::kSeedImuMaxN; out[3] = vc::kSeedImuSearchSteps; out[4] = vc::kSeedImuMoments;
  out[5] = vc::kSeedImuMaxLags;
}

// -2 for what the library refuses as a bad argument
int seed_imu_harness_sweep(int n_frames, const double* frame_t, const double* frame_q, const unsigned char* frame_ok, int n_samples, const double* imu_t,
                           const double* gyro, const double* accel, double max_gap_s, int min_intervals, int n_lags, const double* lags, double* J, double* R,
                           double* bias, int* count, double* moments) {
  const vc::SeedImuData d{n_frames, frame_t, frame_q, frame_ok, n_samples, imu_t, gyro, accel, max_gap_s, min_intervals};
  if (!vc::simu_data_ok(d) || !vc::simu_lags_ok(n_lags, lags)) return -2;
  HostSimu h(d);
  return h.sweep(n_lags, lags, J, R, bias, count, moments);
}

// out[17]: time_offset, R_ck (9), gyro_bias (3), g_dir (2), rms, signal; ints[4]: status, count, the coarse argmin, the coarse lattice's size
int seed_imu_harness_run(int n_frames, const double* frame_t, const double* frame_q, const unsigned char* frame_ok, int n_samples, const double* imu_t,
                         const double* gyro, const double* accel, double max_gap_s, int min_intervals, double range_s, double step_s, int fine, double* out,
                         int* ints, int coarse_cap, double* coarse_lags, double* coarse_J) {
  const vc::SeedImuData d{n_frames, frame_t, frame_q, frame_ok, n_samples, imu_t, gyro, accel, max_gap_s, min_intervals};
  if (!vc::simu_data_ok(d) || !(range_s > 0.0) || fine < 1) return -2;
  HostSimu h(d);
  vc::SeedImuResult r;
  const int rc = vc::simu_pick(h, d, range_s, step_s, fine, &r);
  if (rc != 0) return rc;
  out[0] = r.time_offset;
  std::memcpy(out + 1, r.R_ck, 72); std::memcpy(out + 10, r.gyro_bias, 24); std::memcpy(out + 13, r.g_dir, 16);
  out[15] = r.rms; out[16] = r.signal;
  ints[0] = r.status; ints[1] = r.count; ints[2] = r.coarse_index; ints[3] = r.n_coarse;
  for (int j = 0; j < r.n_coarse && j < coarse_cap; ++j) {
    if (coarse_lags) coarse_lags[j] = r.coarse_lags[(size_t)j];
    if (coarse_J) coarse_J[j] = r.coarse_J[(size_t)j];
  }
  return 0;
}

}  // extern "C"

#ifdef SEED_IMU_HARNESS_MAIN
// a camera turning about two axes, R_ck a 120 degree permutation, a bias and an offset of 30 ms: the seed gives them back
int main() {
  const int nf = 2 * vc::kSeedImuChunk / 16 + 3, ns = 3 * vc::kSeedImuScanBlock + 7;
  const double fdt = 0.05, sdt = fdt * (nf - 1 + 8) / (ns - 1), off = 0.03;
  const double Rck[9] = {0, 1, 0, 0, 0, 1, 1, 0, 0}, bg[3] = {0.002, -0.001, 0.0015};
  auto wc = [](double t, double* w) { w[0] = 0.8 * std::sin(1.7 * t); w[1] = 0.6 * std::cos(2.3 * t + 0.4); w[2] = 0.3 * std::sin(0.9 * t + 1.0); };
  std::vector<double> ft(nf), fq(4 * (size_t)nf), it(ns), gyro(3 * (size_t)ns), accel(3 * (size_t)ns);
  std::vector<unsigned char> ok(nf, 1);
  double q[4] = {0, 0, 0, 1};
  const int sub = 50;
  for (int i = 0; i < nf; ++i) {                             // the rotation integrated in small steps of exp(w h)
    ft[i] = 1.0 + fdt * i;
    std::memcpy(&fq[4 * (size_t)i], q, sizeof(q));
    for (int s = 0; s < sub; ++s) {
      double w[3], dq[4], o[4];
      const double h = fdt / sub;
      wc(ft[i] + (s + 0.5) * h, w);
      const double th = std::sqrt(w[0] * w[0] + w[1] * w[1] + w[2] * w[2]) * h, k = th > 0.0 ? std::sin(0.5 * th) / th * h : 0.5 * h;
      dq[0] = k * w[0]; dq[1] = k * w[1]; dq[2] = k * w[2]; dq[3] = std::cos(0.5 * th);
      vc::quat_mul(q, dq, o);
      std::memcpy(q, o, sizeof(q));
    }
  }
  ok[nf / 2] = 0;
  for (int k = 0; k < ns; ++k) {
    it[k] = 1.0 - 4 * fdt + sdt * k - off;
    double w[3];
    wc(it[k] + off, w);
    for (int c = 0; c < 3; ++c) {
      gyro[3 * (size_t)k + c] = (Rck[c] * w[0] + Rck[3 + c] * w[1] + Rck[6 + c] * w[2]) - bg[c];      // R_ck^T w_c - b_g
      accel[3 * (size_t)k + c] = c == 1 ? 9.8 : 0.01 * w[c];
    }
  }
  double out[17];
  int ints[4];
  std::vector<double> cl(4096), cJ(4096);
  const int rc = seed_imu_harness_run(nf, ft.data(), fq.data(), ok.data(), ns, it.data(), gyro.data(), accel.data(), 0.5, 10, 0.2, 0.0, 8, out, ints, 4096, cl.data(),
                                      cJ.data());
  const double lag1[1] = {out[0]};
  double J1, R1[9], b1[3], m1[vc::kSeedImuMoments];
  int c1 = 0;
  const int rs = seed_imu_harness_sweep(nf, ft.data(), fq.data(), ok.data(), ns, it.data(), gyro.data(), accel.data(), 0.5, 10, 1, lag1, &J1, R1, b1, &c1, m1);
  ft[3] = ft[2];
  const int rb = seed_imu_harness_sweep(nf, ft.data(), fq.data(), ok.data(), ns, it.data(), gyro.data(), accel.data(), 0.5, 10, 1, lag1, &J1, R1, b1, &c1, m1);
  int consts[6];
  seed_imu_harness_constants(consts);
  std::printf("run %d status %d: offset %.6f (truth %.6f), R_ck row 0 %.4f %.4f %.4f, bias %.5f %.5f %.5f, rms %.3e of signal %.3e, %d intervals, %d coarse lags; "
              "sweep %d, count %d; refusal %d\n", rc, ints[0], out[0], off, out[1], out[2], out[3], out[10], out[11], out[12], out[15], out[16], ints[1], ints[3], rs,
              c1, rb);
  const bool good = rc == 0 && ints[0] == 0 && std::fabs(out[0] - off) < 2e-3 && std::fabs(out[2] - 1.0) < 1e-2 && rs == 0 && rb == -2 && c1 == ints[1];
  return good ? 0 : 1;
}
#endif
