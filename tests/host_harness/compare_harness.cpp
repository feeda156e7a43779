// TEST INFRASTRUCTURE: the arithmetic of the calibration comparison (vicalib_amd/csrc/vc_compare.hpp, VC_HD) compiled for the host, so that the
// CPU suite can hold the rays, the fit and the difference sweep against numpy without a GPU.  The Gauss-Newton driver is the very template the
// library runs (cmp_gauss_newton); what the kernels add is the indexing and the order of the sums, which are plain loops in sample order here.
#include <cmath>
#include <cstring>
#include <vector>
#include "../../vicalib_amd/csrc/vc_compare.hpp"

extern "C" {

// One whole run.  fit_out = [R (9) | status | iterations | n_fit | n_left_out | cost0 | cost]; summary = [count, invalid, sum du, sum dv,
// sum |d|^2, max |d|, worst]; rings = n_rings x [count, invalid, sum |d|^2, max |d|].  Returns 0, -6 (VC_ERR_NUMERIC) or -2 (VC_ERR_BAD_ARG).
int vch_run(int model_a, const double* Ka, int nka, int model_b, const double* Kb, int nkb, int w, int h, int gx, int gy, double fit_radius, int max_iters,
            const double* R_ba, int n_rings, double* fit_out, double* diff, unsigned char* flags, double* summary, double* rings) {
  vc::CmpPlan p;
  vc::cmp_plan_set(&p, model_a, Ka, nka, model_b, Kb, nkb, w, h, gx, gy);
  const int n = p.n;
  std::vector<double> rays(3 * (size_t)n), qs(3 * (size_t)n);
  std::vector<unsigned char> f0(n);
  double H[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
  long long n_fit = 0;
  for (int s = 0; s < n; ++s) {
    double b[3];
    vc::cmp_sample(p, s, &qs[3 * s], &qs[3 * s + 1], &qs[3 * s + 2]);
    f0[s] = (unsigned char)vc::cmp_rays(p, qs[3 * s], qs[3 * s + 1], &rays[3 * s], b);
    if (f0[s] == 0 && fit_radius > 0.0 && qs[3 * s + 2] <= fit_radius) {
      ++n_fit;
      for (int r = 0; r < 3; ++r) for (int c = 0; c < 3; ++c) H[3 * r + c] += rays[3 * s + r] * b[c];
    }
  }
  vc::CmpFit f;
  std::memset(&f, 0, sizeof(f));
  double R0[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
  if (fit_radius > 0.0) {
    if (n_fit < 3) return -6;
    vc::rigid_rotation(H, R0);
    const int rc = vc::cmp_gauss_newton([&](const double* R, double* sums) -> int {
      for (int k = 0; k < vc::kCmpFitDoubles; ++k) sums[k] = 0.0;
      for (int s = 0; s < n; ++s) {
        if (f0[s] != 0 || !(qs[3 * s + 2] <= fit_radius)) continue;
        if (vc::cmp_fit_sample(p, R, &rays[3 * s], qs[3 * s], qs[3 * s + 1], sums)) sums[10] += 1.0; else sums[11] += 1.0;
      }
      return 0;
    }, R0, max_iters, &f);
    if (rc != 0) return -6;
    f.n_fit = n_fit;
  } else {
    if (R_ba) { if (!vc::is_rotation(R_ba)) return -2; std::memcpy(R0, R_ba, 72); }
    std::memcpy(f.R, R0, 72);
  }
  std::memcpy(fit_out, f.R, 72);
  fit_out[9] = f.status; fit_out[10] = f.iterations; fit_out[11] = (double)f.n_fit; fit_out[12] = (double)f.n_left_out; fit_out[13] = f.cost0; fit_out[14] = f.cost;
  for (int k = 0; k < 7; ++k) summary[k] = 0.0;
  for (int k = 0; k < 4 * n_rings; ++k) rings[k] = 0.0;
  double best = -1.0; long long best_i = -1;
  std::vector<double> ring_max(n_rings, -1.0);
  for (int s = 0; s < n; ++s) {
    double d[2] = {NAN, NAN};
    const bool valid = f0[s] == 0 && vc::cmp_diff_sample(p, f.R, &rays[3 * s], qs[3 * s], qs[3 * s + 1], d);
    diff[2 * s] = valid ? d[0] : NAN; diff[2 * s + 1] = valid ? d[1] : NAN;
    flags[s] = (unsigned char)(f0[s] | (valid ? 0 : vc::kCmpFlagInvalid));
    double* r = rings + 4 * vc::cmp_ring(qs[3 * s + 2], n_rings);
    if (!valid) { summary[1] += 1.0; r[1] += 1.0; continue; }
    const double sq = vc::cmp_norm2(d[0], d[1]);
    summary[0] += 1.0; summary[2] += d[0]; summary[3] += d[1]; summary[4] += sq;
    if (sq > best) { best = sq; best_i = s; }
    r[0] += 1.0; r[2] += sq;
    double& m = ring_max[vc::cmp_ring(qs[3 * s + 2], n_rings)];
    if (sq > m) m = sq;
  }
  summary[5] = best_i >= 0 ? std::sqrt(best) : 0.0; summary[6] = (double)best_i;
  for (int k = 0; k < n_rings; ++k) rings[4 * k + 3] = ring_max[k] >= 0.0 ? std::sqrt(ring_max[k]) : 0.0;
  return 0;
}

}  // extern "C"
