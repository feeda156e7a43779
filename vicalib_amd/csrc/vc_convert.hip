// vc_convert.hip -- a calibrated camera converted to another camera model on the GPU (gfx950, wave64, fp64).
//
// A vc_converter holds the source camera A, the target model and a lattice of n = gx * gy samples (vc_convert.hpp has the arithmetic and the
// Levenberg-Marquardt driver).  Nothing is allocated beyond the handle's buffers and nothing is launched before the first vc_convert_run.
//
//   k_cvt_rays         one sample per thread: A's Newton inversion (undist_unproject), the unit ray stored, the flag byte (bit 0: the inversion
//                      failed, bit 1: rho > fit_radius) and the workgroup's count of the fit set.  It runs once per handle and again only when a
//                      run asks for another fit radius.
//   k_cvt_fit<MODEL>   one linearisation at K_b: 1024 samples per 256-thread workgroup, a lane takes its four samples in index order and keeps
//                      J^T J packed (nk (nk + 1) / 2), J^T d (nk), E and the two counts in registers -- nk and every index are compile-time
//                      constants of the instantiation.  One instantiation per target model, chosen at the launch through with_model.
//   k_cvt_cost         the values-only sweep, one sample per thread in the shape of k_cmp_diff and through the comparer's cmp_diff_sample at the
//                      identity rotation: E, the counts, and the largest |d|^2 (cmp_norm2) with its sample, the lowest sample on ties.
// The workgroup's record (lat_block_record), the fold of the records (k_lat_reduce) and the handle's device side (LatticeHandle) are the
// lattice core's, vc_lattice.hpp, shared with the comparer and the uncertainty map.
// No floating-point atomic anywhere; the workgroup decomposition depends on n alone: two runs, and two handles, give the same bits.
// One host synchronisation per evaluation of the Levenberg-Marquardt loop and one for each of the two cost sweeps of the readout.  No CPU fallback:
// vc_converter_create fails with VC_ERR_NO_DEVICE without a HIP device.
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstring>
#include "../../include/vicalib_amd.h"
#include "vc_lattice.hpp"
#include "vc_convert.hpp"

namespace {

using vc::CmpPlan;
using vc::CvtCam;
constexpr int kPerWg = 1024;                   // samples of a workgroup of the fit and cost sweeps

struct CvtView {
  CmpPlan plan;                // A, the lattice, the target's model; Kb and pre_b are set per sweep from a CvtCam
  double* rays;                // n x 3: a
  unsigned char* flags;        // n
  double* part;                // workgroup partials of the kernel in flight
};

__global__ __launch_bounds__(256) void k_cvt_rays(CvtView v, double fit_radius) {
  const int s = blockIdx.x * 256 + threadIdx.x;
  double nf[1] = {0.0};
  if (s < v.plan.n) {
    double qx, qy, rho, a[3];
    vc::cmp_sample(v.plan, s, &qx, &qy, &rho);
    // (cmp_rays itself, as k_cmp_rays calls it, so that a is the comparer's a bit for bit; its B half inverts the benign camera of the plan --
    //  the default start -- and is dropped)
    double b[3];
    const int fl = (vc::cmp_rays(v.plan, qx, qy, a, b) & vc::kCmpFlagA) | (rho <= fit_radius ? 0 : vc::kCvtFlagOutside);
    double* dst = v.rays + 3 * (size_t)s;
    dst[0] = a[0]; dst[1] = a[1]; dst[2] = a[2];
    v.flags[s] = (unsigned char)fl;
    if (fl == 0) nf[0] = 1.0;
  }
  vc::lat_block_record(v.part + blockIdx.x, nf);
}

template <int MODEL>
__global__ __launch_bounds__(256) void k_cvt_fit(CvtView v, CvtCam cam) {
  constexpr int NS = vc::cvt_nsums(vc::cvt_nk(MODEL));
  double acc[NS - 2], used = 0.0, left = 0.0;
#pragma unroll
  for (int k = 0; k < NS - 2; ++k) acc[k] = 0.0;
  const int base = blockIdx.x * kPerWg + threadIdx.x;
#pragma unroll 1
  for (int it = 0; it < kPerWg / 256; ++it) {                     // (ascending sample index within a lane)
    const int s = base + it * 256;
    if (s >= v.plan.n || v.flags[s] != 0) continue;
    double qx, qy, rho;
    vc::cmp_sample(v.plan, s, &qx, &qy, &rho);
    const double* src = v.rays + 3 * (size_t)s;
    const double a[3] = {src[0], src[1], src[2]};
    if (vc::cvt_fit_sample<MODEL>(cam, a, qx, qy, acc)) used += 1.0; else left += 1.0;
  }
  double sums[NS];
#pragma unroll
  for (int k = 0; k < NS; ++k) sums[k] = k < NS - 2 ? acc[k] : k == NS - 2 ? used : left;
  vc::lat_block_record(v.part + (size_t)blockIdx.x * NS, sums);
}

// (the shape of k_cmp_diff: one sample per thread, the target in the plan of the kernel argument, the rotation a kernel argument too, d through
//  cmp_diff_sample -- the closest this sweep can come to the code the compiler makes of the comparer's, whose d it is meant to reproduce)
struct CvtRot { double R[9]; };
__global__ __launch_bounds__(256) void k_cvt_cost(CvtView v, CvtRot rot) {
  const int s = blockIdx.x * 256 + threadIdx.x;
  bool in = s < v.plan.n && v.flags[s] == 0, valid = false;
  double d[2] = {0.0, 0.0};
  if (in) {
    double qx, qy, rho;
    vc::cmp_sample(v.plan, s, &qx, &qy, &rho);
    const double* src = v.rays + 3 * (size_t)s;
    const double a[3] = {src[0], src[1], src[2]};
    valid = vc::cmp_diff_sample(v.plan, rot.R, a, qx, qy, d);
  }
  if (!valid) { d[0] = 0.0; d[1] = 0.0; }
  const double sq = vc::cmp_norm2(d[0], d[1]);
  const double sums[3] = {sq, valid ? 1.0 : 0.0, in && !valid ? 1.0 : 0.0};                // E, used, left out
  vc::lat_block_record<3, true>(v.part + (size_t)blockIdx.x * vc::kCvtCostDoubles, sums, valid ? sq : -1.0, valid ? s : -1);
}

}  // namespace

struct vc_converter : vc::LatticeHandle {     // d_buf: [rays | flags | part]
  CvtView v;
  bool have_rays = false, have_run = false;
  double rays_radius = 0.0;            // the fit radius the flags were set for
  long long n_fit = 0;
  vc::CvtFit fit;                      // the last run's
  double max_sq = -1.0;
  long long worst = -1, left_out = 0;
  int nk_a = 0;
  int nk() const { return vc::model_nk(v.plan.model_b); }
  int n_wg_rays() const { return (v.plan.n + 255) / 256; }
  int n_wg() const { return (v.plan.n + kPerWg - 1) / kPerWg; }
};

namespace {

void launch_rays(vc_converter* c, double radius) {
  hipLaunchKernelGGL(k_cvt_rays, dim3(c->n_wg_rays()), dim3(256), 0, c->stream, c->v, radius);
  c->reduce(c->v.part, c->n_wg_rays(), 1, 1);
}
void launch_fit(vc_converter* c, const CvtCam& cam) {
  vc::with_model(c->v.plan.model_b, [&](auto m) {
    hipLaunchKernelGGL(k_cvt_fit<decltype(m)::value>, dim3(c->n_wg()), dim3(256), 0, c->stream, c->v, cam);
  });
  const int ns = vc::cvt_nsums(c->nk());
  c->reduce(c->v.part, c->n_wg(), ns, ns);
}
void launch_cost(vc_converter* c, const CvtCam& cam) {
  CvtView v = c->v;                                                // the target at this point of the fit goes into the plan, where the comparer has its B
  std::memcpy(v.plan.Kb, cam.K, sizeof(cam.K)); v.plan.pre_b = cam.pre;
  const CvtRot rot = {{1, 0, 0, 0, 1, 0, 0, 0, 1}};
  hipLaunchKernelGGL(k_cvt_cost, dim3(c->n_wg_rays()), dim3(256), 0, c->stream, v, rot);
  c->reduce(c->v.part, c->n_wg_rays(), vc::kCvtCostDoubles, vc::kCvtCostDoubles, vc::kCvtCostDoubles - 2);
}

}  // namespace

extern "C" {

int vc_converter_create(int device, int model_a, const double* params_a, int nparams_a, int width, int height, int model_b, int grid_x, int grid_y, vc_converter** out) {
  if (!out || !vc::undist_source_args_ok(model_a, params_a, nparams_a, width, height) || !vc::cvt_model_ok(model_b) ||
      !vc::cvt_grid_ok(width, height, grid_x, grid_y)) return VC_ERR_BAD_ARG;
  vc_converter* c = new vc_converter;
  std::memset(&c->v, 0, sizeof(c->v)); std::memset(&c->fit, 0, sizeof(c->fit));
  c->nk_a = nparams_a;
  double K0[10];
  vc::cvt_default_start(model_b, params_a, K0);                    // (the B of the plan outside a cost sweep: what k_cvt_rays' unused half inverts)
  vc::cmp_plan_set(&c->v.plan, model_a, params_a, nparams_a, model_b, K0, 10, width, height, grid_x, grid_y);
  auto carve = [&](vch::Carver q) {
    const size_t n = (size_t)c->v.plan.n;
    c->v.rays = q.take<double>(n * 3);
    c->v.flags = q.take<unsigned char>(n);
    const size_t fit_part = (size_t)c->n_wg() * vc::kCvtMaxSums, ray_part = (size_t)c->n_wg_rays() * vc::kCvtCostDoubles;      // (rays: 1 per workgroup, cost: 5)
    c->v.part = q.take<double>(fit_part > ray_part ? fit_part : ray_part);
    return q.bytes();
  };
  if (!c->open(device, carve(vch::Carver()), vc::kCvtMaxSums)) { delete c; return VC_ERR_NO_DEVICE; }
  carve(vch::Carver(c->d_buf));
  *out = c;
  return VC_OK;
}
void vc_converter_destroy(vc_converter* c) {
  if (!c) return;
  c->close();
  delete c;
}

int vc_convert_run(vc_converter* c, double fit_radius, int max_iters, const double* start, unsigned free_mask) {
  if (!c || !vc::cvt_run_args_ok(c->v.plan.model_b, fit_radius, start, free_mask)) return VC_ERR_BAD_ARG;
  if (!c->settle()) return VC_ERR_NO_DEVICE;
  c->have_run = false;
  if (!c->have_rays || fit_radius != c->rays_radius) {
    c->have_rays = false;
    launch_rays(c, fit_radius);
    if (!c->fetch(1)) return VC_ERR_NO_DEVICE;
    c->n_fit = (long long)c->h_res[0];
    c->rays_radius = fit_radius; c->have_rays = true;
  }
  const int model_b = c->v.plan.model_b, nk = c->nk();
  double K0[10];
  vc::cvt_default_start(model_b, c->v.plan.Ka, K0);
  if (start) for (int k = 0; k < nk; ++k) K0[k] = start[k];
  const int rc = vc::cvt_levenberg_marquardt([&](const double* K, double* sums) -> int {
    CvtCam cam;
    vc::cvt_cam(model_b, K, &cam);
    launch_fit(c, cam);
    if (!c->fetch(vc::cvt_nsums(nk))) return (int)VC_ERR_NO_DEVICE;
    std::memcpy(sums, c->h_res, (size_t)vc::cvt_nsums(nk) * 8);
    return 0;
  }, nk, K0, free_mask, max_iters, c->n_fit, &c->fit);
  if (rc == -1) return VC_ERR_NUMERIC;
  if (rc != 0) return rc;
  // The readout: values-only sweeps at the start and at K_b.  cost0, cost, the counts and the largest |d| come from them and not from the loop's
  // own sums: the linearisation and the values-only projection round d differently (the compiler contracts them differently), and at a zero
  // residual d is nothing but that rounding -- the comparer of A against the result sums the d of this sweep.
  for (int end = 0; end < 2; ++end) {
    if (end == 1 && std::memcmp(c->fit.K, K0, sizeof(K0)) == 0) { c->fit.cost = c->fit.cost0; break; }      // (no step was accepted)
    CvtCam cam;
    vc::cvt_cam(model_b, end ? c->fit.K : K0, &cam);
    launch_cost(c, cam);
    if (!c->fetch(vc::kCvtCostDoubles)) return VC_ERR_NO_DEVICE;
    (end ? c->fit.cost : c->fit.cost0) = 0.5 * c->h_res[0];
    c->left_out = (long long)c->h_res[2];
    c->max_sq = c->h_res[3]; c->worst = (long long)c->h_res[4];
  }
  c->have_run = true;
  return VC_OK;
}

int vc_convert_get(vc_converter* c, double* params_b, int* nparams_b, int* status, int* iterations, int* n_fit, int* n_left_out, double* cost0, double* cost,
                   double* max_err, long long* worst) {
  if (!c || !c->have_run) return VC_ERR_BAD_ARG;
  const vc::CvtFit& f = c->fit;
  if (params_b) std::memcpy(params_b, f.K, (size_t)c->nk() * 8);
  if (nparams_b) *nparams_b = c->nk();
  if (status) *status = f.status;
  if (iterations) *iterations = f.iterations;
  if (n_fit) *n_fit = (int)f.n_fit;
  if (n_left_out) *n_left_out = (int)c->left_out;
  if (cost0) *cost0 = f.cost0;
  if (cost) *cost = f.cost;
  if (max_err) *max_err = c->worst >= 0 ? std::sqrt(c->max_sq) : 0.0;   // (the host's square root of the largest |d|^2: monotone, so it is the largest |d|)
  if (worst) *worst = c->worst;
  return VC_OK;
}

int vc_convert_comparer(vc_converter* c, vc_comparer** out) {
  if (!c || !out || !c->have_run) return VC_ERR_BAD_ARG;
  const CmpPlan& p = c->v.plan;
  return vc_comparer_create(c->device, p.model_a, p.Ka, c->nk_a, p.model_b, c->fit.K, c->nk(), p.w, p.h, p.gx, p.gy, out);
}

int vc_time_convert(vc_converter* c, int reps, double out_ms[3]) {
  if (!c || reps < 1 || !out_ms || !c->have_run) return VC_ERR_BAD_ARG;
  if (!c->settle()) return VC_ERR_NO_DEVICE;
  CvtCam cam;
  vc::cvt_cam(c->v.plan.model_b, c->fit.K, &cam);
  for (int what = 0; what < 3; ++what) {
    auto launch = [&]() {                                          // (each rewrites what the last run left: the same rays, the same flags)
      if (what == 0) launch_rays(c, c->rays_radius);
      else if (what == 1) launch_fit(c, cam);
      else launch_cost(c, cam);
    };
    const int rc = vch::time_back_to_back(c->stream, reps, launch, &out_ms[what]);
    if (rc != VC_OK) return rc;
  }
  return VC_OK;
}

}  // extern "C"
