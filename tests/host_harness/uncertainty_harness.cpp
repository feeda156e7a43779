// TEST INFRASTRUCTURE: the arithmetic of the projection-uncertainty map (vicalib_amd/csrc/vc_uncertainty.hpp, VC_HD) compiled for the host, so
// that the CPU suite can hold the rays, the implied rotation per parameter and the map against numpy without a GPU.  The argument check, the
// packing of the covariance and the 3 x 3 solve are the very functions the library runs; what the kernels add is the indexing and the order of
// the sums, which are plain loops in sample order here.
#include <cmath>
#include <cstring>
#include <vector>
#include "../../vicalib_amd/csrc/vc_uncertainty.hpp"

namespace {

struct Lattice {
  vc::CmpPlan p;
  std::vector<double> rays, qs;            // n x 3: a; n x 3: qx, qy, rho
  std::vector<unsigned char> f0;
};
template <int MODEL>
void gram_sweep(const Lattice& L, double fit_radius, double* sums) {
  constexpr int ns = vc::unc_ngram(vc::cvt_nk(MODEL));
  for (int s = 0; s < L.p.n; ++s)
    if (L.f0[s] == 0 && L.qs[3 * s + 2] <= fit_radius && vc::unc_gram_sample<MODEL>(L.p, &L.rays[3 * s], sums)) sums[ns - 1] += 1.0;
}
template <int MODEL>
void map_sweep(const Lattice& L, const vc::UncFit& fit, const vc::UncCov& cov, double* sigma, unsigned char* flags) {
  for (int s = 0; s < L.p.n; ++s) {
    double sg[3];
    const bool valid = L.f0[s] == 0 && vc::unc_sigma_sample<MODEL>(L.p, &L.rays[3 * s], fit, cov, sg);
    for (int k = 0; k < 3; ++k) sigma[3 * s + k] = valid ? sg[k] : NAN;
    flags[s] = (unsigned char)(L.f0[s] | (valid ? 0 : vc::kCmpFlagInvalid));
  }
}

}  // namespace

extern "C" {

// the shared argument check of a run on its own
int vch_uncertainty_args_ok(const double* cov, int nk, double sigma_px, double fit_radius) { return vc::unc_run_args_ok(cov, nk, sigma_px, fit_radius) ? 1 : 0; }

// One whole run.  fit_out = [M (30: 3 x nk) | G (9) | n_fit]; sigma = n x 3; summary = [count, invalid, sum var, max lam, worst];
// rings = n_rings x [count, invalid, sum var, max lam].  Returns 0, -6 (VC_ERR_NUMERIC) or -2 (VC_ERR_BAD_ARG).
int vch_uncertainty(int model, const double* K, int nk, int w, int h, int gx, int gy, const double* cov, double sigma_px, double fit_radius, int n_rings,
                    double* fit_out, double* sigma, unsigned char* flags, double* summary, double* rings) {
  if (!vc::cvt_model_ok(model) || nk != vc::model_nk(model) || !vc::cvt_grid_ok(w, h, gx, gy) || n_rings < 1 || n_rings > vc::kCmpMaxRings) return -2;
  if (!vc::unc_run_args_ok(cov, nk, sigma_px, fit_radius)) return -2;
  Lattice L;
  vc::CmpPlan& p = L.p;
  vc::cmp_plan_set(&p, model, K, nk, model, K, nk, w, h, gx, gy);      // (B is A again)
  const int n = p.n;
  L.rays.resize(3 * (size_t)n); L.qs.resize(3 * (size_t)n); L.f0.resize(n);
  for (int s = 0; s < n; ++s) {
    vc::cmp_sample(p, s, &L.qs[3 * s], &L.qs[3 * s + 1], &L.qs[3 * s + 2]);
    L.f0[s] = (unsigned char)vc::cvt_ray(p, L.qs[3 * s], L.qs[3 * s + 1], &L.rays[3 * s]);
  }
  vc::UncFit fit;
  std::memset(&fit, 0, sizeof(fit));
  double G[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
  long long n_fit = 0;
  if (fit_radius > 0.0) {
    double sums[vc::kUncMaxGram];
    for (int k = 0; k < vc::kUncMaxGram; ++k) sums[k] = 0.0;
    vc::with_model(model, [&](auto m) { gram_sweep<decltype(m)::value>(L, fit_radius, sums); });
    if (!vc::unc_solve_fit(sums, nk, &fit, G, &n_fit)) return -6;
  }
  std::memcpy(fit_out, fit.M, 240); std::memcpy(fit_out + 30, G, 72); fit_out[39] = (double)n_fit;
  vc::UncCov pc;
  vc::unc_pack_cov(cov, nk, sigma_px, &pc);
  vc::with_model(model, [&](auto m) { map_sweep<decltype(m)::value>(L, fit, pc, sigma, flags); });
  for (int k = 0; k < 5; ++k) summary[k] = 0.0;
  for (int k = 0; k < 4 * n_rings; ++k) rings[k] = 0.0;
  double best = -1.0; long long best_i = -1;
  std::vector<double> ring_max(n_rings, -1.0);
  for (int s = 0; s < n; ++s) {
    const int ring = vc::cmp_ring(L.qs[3 * s + 2], n_rings);
    double* r = rings + 4 * ring;
    if (flags[s] & vc::kCmpFlagInvalid) { summary[1] += 1.0; r[1] += 1.0; continue; }
    const double var = vc::unc_var(&sigma[3 * s]), lam = vc::unc_lam(&sigma[3 * s]);
    summary[0] += 1.0; summary[2] += var;
    if (lam > best) { best = lam; best_i = s; }
    r[0] += 1.0; r[2] += var;
    if (lam > ring_max[ring]) ring_max[ring] = lam;
  }
  summary[3] = best_i >= 0 ? best : 0.0; summary[4] = (double)best_i;
  for (int k = 0; k < n_rings; ++k) rings[4 * k + 3] = ring_max[k] >= 0.0 ? ring_max[k] : 0.0;
  return 0;
}

}  // extern "C"
