// vc_uncertainty.hip -- the projection uncertainty of one calibrated camera mapped over its image on the GPU (gfx950, wave64, fp64).
//
// A vc_uncertainty holds camera A and a lattice of n = gx * gy samples (vc_uncertainty.hpp has the arithmetic).  Nothing is allocated beyond
// the handle's buffers and nothing is launched before the first vc_uncertainty_run.
//
//   k_unc_rays          one sample per thread: A's Newton inversion through cmp_rays (as k_cvt_rays takes it: a is the comparer's a bit for
//                       bit), the unit ray and the inversion flag stored.  Once per handle.
//   k_unc_gram<MODEL>   the sums of the implied rotation per parameter: 1024 samples per 256-thread workgroup, a lane takes its four samples
//                       in index order and keeps G (6 packed), C (3 nk) and the size of the fit set in registers -- nk and every index are
//                       compile-time constants of the instantiation.  Again only when a run asks for another fit radius.
//   k_unc_map<MODEL>    one sample per thread, M (3 x nk) and the packed, pre-scaled covariance as kernel arguments: Sigma = J Cov J^T with
//                       J = B + Jw M, the triple (s_uu, s_uv, s_vv) and the flags stored, then the workgroup's partial of the summary and of
//                       the rings (unc_block_sums).
//   k_unc_rings         the same partials at another ring count from the stored triples: no inversion, no projection.
// The workgroup's record (lat_block_record), the rings (lat_ring_walk), the fold of the records (k_lat_reduce) and the handle's device side
// (LatticeHandle) are the lattice core's, vc_lattice.hpp, shared with the comparer and the converter.
// One instantiation per model, chosen at the launch through with_model.  No floating-point atomic anywhere; the workgroup decomposition
// depends on n alone: two runs, and two handles, give the same bits.  One host synchronisation per sweep.  No CPU fallback:
// vc_uncertainty_create fails with VC_ERR_NO_DEVICE without a HIP device.
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstring>
#include <vector>
#include "../../include/vicalib_amd.h"
#include "vc_lattice.hpp"
#include "vc_uncertainty.hpp"

namespace {

using vc::CmpPlan;
using vc::UncCov;
using vc::UncFit;
constexpr int kPerWg = 1024;                                                          // samples of a workgroup of the Gram sweep
constexpr int kMapDoubles = vc::kUncSumDoubles + vc::kUncRingDoubles * vc::kCmpMaxRings;   // a workgroup's record of the map sweep
static_assert(vc::kUncRingDoubles == vc::kLatRingDoubles, "a ring's record is the lattice core's");

struct UncView {
  CmpPlan plan;                // A and the lattice (B is A again: the half of cmp_rays that is dropped)
  double* rays;                // n x 3: a
  unsigned char* flags0;       // n: bit 0, as k_unc_rays left it
  unsigned char* flags;        // n: the last map sweep's, bit 2 added
  double* sigma;               // n x 3: s_uu, s_uv, s_vv
  double* part;                // workgroup partials of the kernel in flight
};

__global__ __launch_bounds__(256) void k_unc_rays(UncView v) {
  const int s = blockIdx.x * 256 + threadIdx.x;
  if (s >= v.plan.n) return;
  double qx, qy, rho, a[3], b[3];
  vc::cmp_sample(v.plan, s, &qx, &qy, &rho);
  const int fl = vc::cmp_rays(v.plan, qx, qy, a, b) & vc::kCmpFlagA;
  double* dst = v.rays + 3 * (size_t)s;
  dst[0] = a[0]; dst[1] = a[1]; dst[2] = a[2];
  v.flags0[s] = (unsigned char)fl;
}

template <int MODEL>
__global__ __launch_bounds__(256) void k_unc_gram(UncView v, double fit_radius) {
  constexpr int NS = vc::unc_ngram(vc::cvt_nk(MODEL));
  double acc[NS - 1], nf = 0.0;
#pragma unroll
  for (int k = 0; k < NS - 1; ++k) acc[k] = 0.0;
  const int base = blockIdx.x * kPerWg + threadIdx.x;
#pragma unroll 1
  for (int it = 0; it < kPerWg / 256; ++it) {                     // (ascending sample index within a lane)
    const int s = base + it * 256;
    if (s >= v.plan.n || v.flags0[s] != 0) continue;
    double qx, qy, rho;
    vc::cmp_sample(v.plan, s, &qx, &qy, &rho);
    if (!(rho <= fit_radius)) continue;
    const double* src = v.rays + 3 * (size_t)s;
    const double a[3] = {src[0], src[1], src[2]};
    if (vc::unc_gram_sample<MODEL>(v.plan, a, acc)) nf += 1.0;
  }
  double sums[NS];
#pragma unroll
  for (int k = 0; k < NS; ++k) sums[k] = k < NS - 1 ? acc[k] : nf;
  vc::lat_block_record(v.part + (size_t)blockIdx.x * NS, sums);
}

// The workgroup's record of the map sweep from one sample per thread: `in` (the thread has a sample), `valid`, var and lam (0 unless valid),
// ring (-1 without a sample): count, invalid, sum var, the largest lam and its sample, then the rings, where var is summed and lam is the
// key.  Reached by every thread of the workgroup.
__device__ __forceinline__ void unc_block_sums(double* rec, int s, bool in, bool valid, double var, double lam, int ring, int n_rings) {
  __shared__ double s_var[256], s_lam[256];      // s_lam: -1 of an invalid sample
  __shared__ int s_ring[256];
  s_var[threadIdx.x] = var;
  s_lam[threadIdx.x] = valid ? lam : -1.0;
  s_ring[threadIdx.x] = ring;
  const double sums[3] = {valid ? 1.0 : 0.0, in && !valid ? 1.0 : 0.0, var};
  vc::lat_block_record<3, true>(rec, sums, valid ? lam : -1.0, valid ? s : -1);
  vc::lat_ring_walk(rec + vc::kUncSumDoubles, n_rings, s_ring, s_var, s_lam);
}

template <int MODEL>
__global__ __launch_bounds__(256) void k_unc_map(UncView v, UncFit fit, UncCov cov, int n_rings) {
  const int s = blockIdx.x * 256 + threadIdx.x;
  const double nan = __builtin_nan("");
  const bool in = s < v.plan.n;
  bool valid = false;
  double sg[3] = {0.0, 0.0, 0.0};
  int ring = -1;
  if (in) {
    double qx, qy, rho;
    vc::cmp_sample(v.plan, s, &qx, &qy, &rho);
    ring = vc::cmp_ring(rho, n_rings);
    const int f0 = v.flags0[s];
    if (f0 == 0) {
      const double* src = v.rays + 3 * (size_t)s;
      const double a[3] = {src[0], src[1], src[2]};
      valid = vc::unc_sigma_sample<MODEL>(v.plan, a, fit, cov, sg);
    }
    double* dst = v.sigma + 3 * (size_t)s;
    dst[0] = valid ? sg[0] : nan; dst[1] = valid ? sg[1] : nan; dst[2] = valid ? sg[2] : nan;
    v.flags[s] = (unsigned char)(f0 | (valid ? 0 : vc::kCmpFlagInvalid));
  }
  if (!valid) { sg[0] = 0.0; sg[1] = 0.0; sg[2] = 0.0; }
  unc_block_sums(v.part + (size_t)blockIdx.x * kMapDoubles, s, in, valid, vc::unc_var(sg), vc::unc_lam(sg), ring, n_rings);
}

__global__ __launch_bounds__(256) void k_unc_rings(UncView v, int n_rings) {
  const int s = blockIdx.x * 256 + threadIdx.x;
  const bool in = s < v.plan.n;
  bool valid = false;
  double sg[3] = {0.0, 0.0, 0.0};
  int ring = -1;
  if (in) {
    double qx, qy, rho;
    vc::cmp_sample(v.plan, s, &qx, &qy, &rho);
    ring = vc::cmp_ring(rho, n_rings);
    valid = (v.flags[s] & vc::kCmpFlagInvalid) == 0;
    if (valid) { const double* src = v.sigma + 3 * (size_t)s; sg[0] = src[0]; sg[1] = src[1]; sg[2] = src[2]; }
  }
  unc_block_sums(v.part + (size_t)blockIdx.x * kMapDoubles, s, in, valid, vc::unc_var(sg), vc::unc_lam(sg), ring, n_rings);
}

}  // namespace

struct vc_uncertainty : vc::LatticeHandle {   // d_buf: [rays | sigma | flags0 | flags | part]
  UncView v;
  bool have_rays = false, have_gram = false, have_run = false, have_cal_cov = false;
  double gram_radius = 0.0;            // the fit radius G, C and M were made for
  UncFit gram_fit;                     // ... and their M, G and fit set
  double gram_G[9];
  long long gram_n_fit = 0;
  double cal_cov[100];                 // the calibrator's covariance of this camera's intrinsics (vc_uncertainty_create_for_camera)
  UncFit fit;                          // the last run's (zero without compensation)
  UncCov cov;
  double G[9];
  long long n_fit = 0;
  double fit_radius = 0.0;
  double summary[kMapDoubles];         // the last run's, rings at kCmpDefaultRings
  int rings_n = 0;                     // ring count of `rings` (a rings-only sweep), 0 = none
  double rings[vc::kUncRingDoubles * vc::kCmpMaxRings];
  int nk() const { return vc::model_nk(v.plan.model_a); }
  int n_wg() const { return (v.plan.n + 255) / 256; }
  int n_wg_gram() const { return (v.plan.n + kPerWg - 1) / kPerWg; }
};

namespace {

void launch_rays(vc_uncertainty* u) { hipLaunchKernelGGL(k_unc_rays, dim3(u->n_wg()), dim3(256), 0, u->stream, u->v); }
void launch_gram(vc_uncertainty* u, double radius) {
  const int ns = vc::unc_ngram(u->nk());
  vc::with_model(u->v.plan.model_a, [&](auto m) {
    hipLaunchKernelGGL(k_unc_gram<decltype(m)::value>, dim3(u->n_wg_gram()), dim3(256), 0, u->stream, u->v, radius);
  });
  u->reduce(u->v.part, u->n_wg_gram(), ns, ns);
}
void launch_map(vc_uncertainty* u, const UncFit& fit, const UncCov& cov, int n_rings, bool rings_only) {
  if (rings_only) hipLaunchKernelGGL(k_unc_rings, dim3(u->n_wg()), dim3(256), 0, u->stream, u->v, n_rings);
  else vc::with_model(u->v.plan.model_a, [&](auto m) {
    hipLaunchKernelGGL(k_unc_map<decltype(m)::value>, dim3(u->n_wg()), dim3(256), 0, u->stream, u->v, fit, cov, n_rings);
  });
  u->reduce(u->v.part, u->n_wg(), kMapDoubles, vc::kUncSumDoubles + vc::kUncRingDoubles * n_rings, vc::kUncSumDoubles - 2, vc::kUncSumDoubles);
}

}  // namespace

void vc::unc_attach_cov(vc_uncertainty* u, const double* cov) {
  const int nk = u->nk();
  std::memcpy(u->cal_cov, cov, (size_t)nk * nk * 8);
  u->have_cal_cov = true;
}

extern "C" {

int vc_uncertainty_create(int device, int model, const double* params, int nparams, int width, int height, int grid_x, int grid_y, vc_uncertainty** out) {
  if (!out || !vc::undist_source_args_ok(model, params, nparams, width, height) || !vc::cvt_grid_ok(width, height, grid_x, grid_y)) return VC_ERR_BAD_ARG;
  vc_uncertainty* u = new vc_uncertainty;
  std::memset(&u->v, 0, sizeof(u->v)); std::memset(&u->fit, 0, sizeof(u->fit)); std::memset(&u->cov, 0, sizeof(u->cov));
  std::memset(&u->gram_fit, 0, sizeof(u->gram_fit));
  vc::cmp_plan_set(&u->v.plan, model, params, nparams, model, params, nparams, width, height, grid_x, grid_y);      // (B is A again)
  auto carve = [&](vch::Carver q) {
    const size_t n = (size_t)u->v.plan.n;
    u->v.rays = q.take<double>(n * 3);
    u->v.sigma = q.take<double>(n * 3);
    u->v.flags0 = q.take<unsigned char>(n);
    u->v.flags = q.take<unsigned char>(n);
    const size_t gram_part = (size_t)u->n_wg_gram() * vc::kUncMaxGram, map_part = (size_t)u->n_wg() * kMapDoubles;
    u->v.part = q.take<double>(gram_part > map_part ? gram_part : map_part);
    return q.bytes();
  };
  if (!u->open(device, carve(vch::Carver()), kMapDoubles)) { delete u; return VC_ERR_NO_DEVICE; }
  carve(vch::Carver(u->d_buf));
  *out = u;
  return VC_OK;
}
void vc_uncertainty_destroy(vc_uncertainty* u) {
  if (!u) return;
  u->close();
  delete u;
}

int vc_uncertainty_run(vc_uncertainty* u, const double* cov, double sigma_px, double fit_radius) {
  if (!u) return VC_ERR_BAD_ARG;
  u->have_run = false; u->rings_n = 0;                             // a refused run leaves nothing to read
  if (!cov && !u->have_cal_cov) return VC_ERR_BAD_ARG;
  const double* c = cov ? cov : u->cal_cov;
  const int nk = u->nk();
  if (!vc::unc_run_args_ok(c, nk, sigma_px, fit_radius)) return VC_ERR_BAD_ARG;
  if (!u->settle()) return VC_ERR_NO_DEVICE;
  if (!u->have_rays) {
    launch_rays(u);
    if (!u->fetch(0)) return VC_ERR_NO_DEVICE;
    u->have_rays = true;
  }
  if (fit_radius > 0.0) {
    if (!u->have_gram || fit_radius != u->gram_radius) {
      u->have_gram = false;
      const int ns = vc::unc_ngram(nk);
      launch_gram(u, fit_radius);
      if (!u->fetch(ns)) return VC_ERR_NO_DEVICE;
      if (!vc::unc_solve_fit(u->h_res, nk, &u->gram_fit, u->gram_G, &u->gram_n_fit)) return VC_ERR_NUMERIC;
      u->gram_radius = fit_radius; u->have_gram = true;
    }
    u->fit = u->gram_fit; u->n_fit = u->gram_n_fit;
    std::memcpy(u->G, u->gram_G, sizeof(u->G));
  } else {                                                         // no compensation: M = 0, J = B
    std::memset(&u->fit, 0, sizeof(u->fit)); std::memset(u->G, 0, sizeof(u->G));
    u->n_fit = 0;
  }
  vc::unc_pack_cov(c, nk, sigma_px, &u->cov);
  launch_map(u, u->fit, u->cov, vc::kCmpDefaultRings, false);
  const int m = vc::kUncSumDoubles + vc::kUncRingDoubles * vc::kCmpDefaultRings;
  if (!u->fetch(m)) return VC_ERR_NO_DEVICE;
  std::memcpy(u->summary, u->h_res, (size_t)m * 8);
  u->fit_radius = fit_radius;
  u->have_run = true;
  return VC_OK;
}

int vc_uncertainty_get_fit(vc_uncertainty* u, double* M, double* G, int* n_fit) {
  if (!u || !u->have_run) return VC_ERR_BAD_ARG;
  if (M) std::memcpy(M, u->fit.M, (size_t)3 * u->nk() * 8);
  if (G) std::memcpy(G, u->G, 72);
  if (n_fit) *n_fit = (int)u->n_fit;
  return VC_OK;
}

int vc_uncertainty_get_map(vc_uncertainty* u, double* sigma, unsigned char* flags) {
  if (!u || !u->have_run) return VC_ERR_BAD_ARG;
  if (!sigma && !flags) return VC_OK;
  if (hipSetDevice(u->device) != hipSuccess || hipStreamSynchronize(u->stream) != hipSuccess) return VC_ERR_NO_DEVICE;
  const size_t n = (size_t)u->v.plan.n;
  if (sigma && hipMemcpy(sigma, u->v.sigma, n * 24, hipMemcpyDeviceToHost) != hipSuccess) return VC_ERR_NO_DEVICE;
  if (flags && hipMemcpy(flags, u->v.flags, n, hipMemcpyDeviceToHost) != hipSuccess) return VC_ERR_NO_DEVICE;
  return VC_OK;
}

int vc_uncertainty_summary(vc_uncertainty* u, long long* count, long long* invalid, double* sum_var, double* max_lam, long long* worst) {
  if (!u || !u->have_run) return VC_ERR_BAD_ARG;
  const double* s = u->summary;
  if (count) *count = (long long)s[0];
  if (invalid) *invalid = (long long)s[1];
  if (sum_var) *sum_var = s[2];
  if (max_lam) *max_lam = s[4] >= 0.0 ? s[3] : 0.0;
  if (worst) *worst = (long long)s[4];
  return VC_OK;
}

int vc_uncertainty_rings(vc_uncertainty* u, int n_rings, long long* count, long long* invalid, double* sum_var, double* max_lam) {
  if (!u || !u->have_run || n_rings < 1 || n_rings > vc::kCmpMaxRings) return VC_ERR_BAD_ARG;
  const double* r = u->summary + vc::kUncSumDoubles;
  if (n_rings != vc::kCmpDefaultRings) {
    if (u->rings_n != n_rings) {                                   // a rings-only sweep over the stored triples
      if (hipSetDevice(u->device) != hipSuccess) return VC_ERR_NO_DEVICE;
      u->rings_n = 0;
      launch_map(u, u->fit, u->cov, n_rings, true);
      if (!u->fetch(vc::kUncSumDoubles + vc::kUncRingDoubles * n_rings)) return VC_ERR_NO_DEVICE;
      std::memcpy(u->rings, u->h_res + vc::kUncSumDoubles, (size_t)vc::kUncRingDoubles * n_rings * 8);
      u->rings_n = n_rings;
    }
    r = u->rings;
  }
  for (int k = 0; k < n_rings; ++k) {
    const double* q = r + vc::kUncRingDoubles * k;
    if (count) count[k] = (long long)q[0];
    if (invalid) invalid[k] = (long long)q[1];
    if (sum_var) sum_var[k] = q[2];
    if (max_lam) max_lam[k] = q[0] > 0.0 ? q[3] : 0.0;
  }
  return VC_OK;
}

int vc_time_uncertainty(vc_uncertainty* u, int reps, double out_ms[3]) {
  if (!u || reps < 1 || !out_ms || !u->have_run) return VC_ERR_BAD_ARG;
  if (!u->settle()) return VC_ERR_NO_DEVICE;
  for (int what = 0; what < 3; ++what) {
    auto launch = [&]() {                                          // (each rewrites what the last run left: the same rays, the same map)
      if (what == 0) launch_rays(u);
      else if (what == 1) launch_gram(u, u->fit_radius > 0.0 ? u->fit_radius : 1e300);
      else launch_map(u, u->fit, u->cov, vc::kCmpDefaultRings, false);
    };
    const int rc = vch::time_back_to_back(u->stream, reps, launch, &out_ms[what]);
    if (rc != VC_OK) return rc;
  }
  return VC_OK;
}

}  // extern "C"
