// TEST INFRASTRUCTURE: the arithmetic of the camera-model conversion (vicalib_amd/csrc/vc_convert.hpp, VC_HD) compiled for the host, so that the
// CPU suite can hold the rays, the fit and the cost sweep against numpy without a GPU.  The Levenberg-Marquardt driver is the very template the
// library runs (cvt_levenberg_marquardt); what the kernels add is the indexing and the order of the sums, which are plain loops in sample order here.
#include <cmath>
#include <cstring>
#include <vector>
#include "../../vicalib_amd/csrc/vc_convert.hpp"

namespace {

struct Lattice {
  vc::CmpPlan p;
  std::vector<double> rays, qs;            // n x 3: a; n x 3: qx, qy, rho
  std::vector<unsigned char> flags;
  long long n_fit = 0;
};
void make_lattice(Lattice* L, int model_a, const double* Ka, int nka, int w, int h, int model_b, int gx, int gy, double fit_radius) {
  vc::CmpPlan& p = L->p;
  double K0[10];
  vc::cvt_default_start(model_b, Ka, K0);                          // (the plan's B outside a cost sweep, as the library has it)
  vc::cmp_plan_set(&p, model_a, Ka, nka, model_b, K0, 10, w, h, gx, gy);
  const int n = p.n;
  L->rays.resize(3 * (size_t)n); L->qs.resize(3 * (size_t)n); L->flags.resize(n);
  for (int s = 0; s < n; ++s) {
    vc::cmp_sample(p, s, &L->qs[3 * s], &L->qs[3 * s + 1], &L->qs[3 * s + 2]);
    L->flags[s] = (unsigned char)(vc::cvt_ray(p, L->qs[3 * s], L->qs[3 * s + 1], &L->rays[3 * s]) | (L->qs[3 * s + 2] <= fit_radius ? 0 : vc::kCvtFlagOutside));
    if (L->flags[s] == 0) ++L->n_fit;
  }
}
template <int MODEL>
void fit_sweep(const Lattice& L, const vc::CvtCam& cam, double* sums) {
  constexpr int ns = vc::cvt_nsums(vc::cvt_nk(MODEL));
  for (int s = 0; s < L.p.n; ++s)
    if (L.flags[s] == 0) sums[vc::cvt_fit_sample<MODEL>(cam, &L.rays[3 * s], L.qs[3 * s], L.qs[3 * s + 1], sums) ? ns - 2 : ns - 1] += 1.0;
}

}  // namespace

extern "C" {

// One whole conversion.  out = [K_b (10) | status | iterations | n_fit | n_left_out | cost0 | cost | max |d| | worst].
// Returns 0, -6 (VC_ERR_NUMERIC) or -2 (VC_ERR_BAD_ARG).
int vch_convert(int model_a, const double* Ka, int nka, int w, int h, int model_b, int gx, int gy, double fit_radius, int max_iters, const double* start,
                unsigned free_mask, double* out) {
  if (!vc::cvt_model_ok(model_a) || !vc::cvt_model_ok(model_b) || nka != vc::model_nk(model_a) || !vc::cvt_grid_ok(w, h, gx, gy)) return -2;
  if (!vc::cvt_run_args_ok(model_b, fit_radius, start, free_mask)) return -2;
  Lattice L;
  make_lattice(&L, model_a, Ka, nka, w, h, model_b, gx, gy, fit_radius);
  const int nk = vc::model_nk(model_b);
  double K0[10];
  vc::cvt_default_start(model_b, Ka, K0);
  if (start) for (int k = 0; k < nk; ++k) K0[k] = start[k];
  vc::CvtFit f;
  const int rc = vc::cvt_levenberg_marquardt([&](const double* K, double* sums) -> int {
    vc::CvtCam cam;
    vc::cvt_cam(model_b, K, &cam);
    for (int k = 0; k < vc::cvt_nsums(nk); ++k) sums[k] = 0.0;
    vc::with_model(model_b, [&](auto m) { fit_sweep<decltype(m)::value>(L, cam, sums); });
    return 0;
  }, nk, K0, free_mask, max_iters, L.n_fit, &f);
  if (rc != 0) return -6;
  // the readout: the cost sweep at the start and at K_b, as the library takes cost0, cost, the counts and the largest |d|
  double best = -1.0; long long best_i = -1, left = 0;
  for (int end = 0; end < 2; ++end) {
    vc::CvtCam cam;
    vc::cvt_cam(model_b, end ? f.K : K0, &cam);
    vc::CmpPlan p = L.p;
    std::memcpy(p.Kb, cam.K, sizeof(cam.K)); p.pre_b = cam.pre;
    double e = 0.0;
    best = -1.0; best_i = -1; left = 0;
    for (int s = 0; s < p.n; ++s) {
      if (L.flags[s] != 0) continue;
      double sq;
      if (!vc::cvt_cost_sample(p, &L.rays[3 * s], L.qs[3 * s], L.qs[3 * s + 1], &sq)) { ++left; continue; }
      e += sq;
      if (sq > best) { best = sq; best_i = s; }
    }
    (end ? f.cost : f.cost0) = 0.5 * e;
  }
  std::memcpy(out, f.K, 80);
  out[10] = f.status; out[11] = f.iterations; out[12] = (double)f.n_fit; out[13] = (double)left; out[14] = f.cost0; out[15] = f.cost;
  out[16] = best_i >= 0 ? std::sqrt(best) : 0.0; out[17] = (double)best_i;
  return 0;
}

// The comparer's difference sweep of A against (model_b, Kb) at the identity rotation over the whole lattice, in its arithmetic (cmp_rays,
// cmp_diff_sample, cmp_norm2): out = [count, sum |d|^2, max |d|, worst].
int vch_convert_compare(int model_a, const double* Ka, int nka, int w, int h, int model_b, const double* Kb, int nkb, int gx, int gy, double* out) {
  vc::CmpPlan p;
  vc::cmp_plan_set(&p, model_a, Ka, nka, model_b, Kb, nkb, w, h, gx, gy);
  const double I[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
  double count = 0.0, sum = 0.0, best = -1.0; long long best_i = -1;
  for (int s = 0; s < p.n; ++s) {
    double qx, qy, rho, a[3], b[3], d[2];
    vc::cmp_sample(p, s, &qx, &qy, &rho);
    if (vc::cmp_rays(p, qx, qy, a, b) != 0 || !vc::cmp_diff_sample(p, I, a, qx, qy, d)) continue;
    const double sq = vc::cmp_norm2(d[0], d[1]);
    count += 1.0; sum += sq;
    if (sq > best) { best = sq; best_i = s; }
  }
  out[0] = count; out[1] = sum; out[2] = best_i >= 0 ? std::sqrt(best) : 0.0; out[3] = (double)best_i;
  return 0;
}

}  // extern "C"
