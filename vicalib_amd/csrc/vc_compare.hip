// vc_compare.hip -- two calibrations of one camera compared in pixel space on the GPU (gfx950, wave64, fp64).
//
// A vc_comparer holds cameras A and B of one image size and a lattice of n = gx * gy samples (vc_compare.hpp has the arithmetic).  Nothing is
// allocated beyond the handle's buffers and nothing is launched before the first vc_compare_run.
//
//   k_cmp_rays    one sample per thread: both Newton inversions (undist_unproject), the unit ray a stored, the inversion flags, and the
//                 workgroup's partial of Horn's H = sum over the fit set of a b^T with the size of the fit set.  It runs once per handle and
//                 again only when a run asks for another fit radius (the fit set is part of H).
//   k_cmp_fit     one Gauss-Newton evaluation at a rotation R: 1024 samples per 256-thread workgroup, a lane takes its four samples in index
//                 order and keeps J^T J (6), J^T d (3), E and the two counts in registers; wave_allsum, then the four waves' sums in wave
//                 order -> one partial record per workgroup.
//   k_cmp_diff    the difference sweep at the final R, one sample per thread: d and the flags stored, the workgroup's partial of the summary
//                 (the maximum by the xor butterfly that keeps the lower index) and of the rings.  The rings are built in LDS: every thread
//                 leaves its ring and |d|^2 there, then thread k adds up ring k's entries in thread order.  With rings_only it reads the
//                 stored d instead of computing it: vc_compare_rings at another ring count inverts and projects nothing.
//   k_cmp_reduce  one wavefront: lane c adds column c of the workgroup partials in workgroup order (maxima: the first of equal ones).
// No floating-point atomic anywhere; the workgroup decomposition depends on n alone: two runs, and two handles, give the same bits.
// One host synchronisation per Gauss-Newton evaluation and one for the difference sweep.  No CPU fallback: vc_comparer_create fails with
// VC_ERR_NO_DEVICE without a HIP device.  vc_compare_extrinsics is host code and needs none.
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstring>
#include <vector>
#include "../../include/vicalib_amd.h"
#include "vc_kutil.hpp"
#include "vc_hostutil.hpp"
#include "vc_compare.hpp"

namespace {

using vc::CmpPlan;
constexpr int kFitPerWg = 1024;
constexpr int kRayDoubles = 10;                                                       // H (9), size of the fit set
constexpr int kDiffDoubles = vc::kCmpSumDoubles + vc::kCmpRingDoubles * vc::kCmpMaxRings;   // a workgroup's record of the difference sweep
enum { kReduceSums = 0, kReduceDiff = 1 };

struct CmpView {
  CmpPlan plan;
  double* rays;                // n x 3: a
  unsigned char* flags0;       // n: bits 0 and 1, as k_cmp_rays left them
  unsigned char* flags;        // n: the last difference sweep's, bit 2 added
  double2* diff;               // n
  double* part;                // workgroup partials of the kernel in flight
  double* out;                 // the reduced record
};
struct CmpRot { double R[9]; };

// the four waves' values of `x` (the same in every lane of a wave) added in wave order; the result in every thread.  `slot` separates the
// uses within one kernel.
__device__ __forceinline__ void block_stage(double (*s)[16], int slot, double x) {
  if ((threadIdx.x & 63) == 0) s[threadIdx.x >> 6][slot] = x;
}
__device__ __forceinline__ double block_total(double (*s)[16], int slot) { return ((s[0][slot] + s[1][slot]) + s[2][slot]) + s[3][slot]; }

__global__ __launch_bounds__(256) void k_cmp_rays(CmpView v, double fit_radius) {
  __shared__ double s_w[4][16];
  const int s = blockIdx.x * 256 + threadIdx.x;
  double H[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0}, nf = 0.0;
  if (s < v.plan.n) {
    double qx, qy, rho, a[3], b[3];
    vc::cmp_sample(v.plan, s, &qx, &qy, &rho);
    const int fl = vc::cmp_rays(v.plan, qx, qy, a, b);
    double* dst = v.rays + 3 * (size_t)s;
    dst[0] = a[0]; dst[1] = a[1]; dst[2] = a[2];
    v.flags0[s] = (unsigned char)fl;
    if (fl == 0 && rho <= fit_radius) {
      nf = 1.0;
#pragma unroll
      for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c) H[3 * r + c] = a[r] * b[c];
    }
  }
#pragma unroll
  for (int k = 0; k < 9; ++k) block_stage(s_w, k, vc::wave_allsum(H[k]));
  block_stage(s_w, 9, vc::wave_allsum(nf));
  __syncthreads();
  if (threadIdx.x < kRayDoubles) v.part[(size_t)blockIdx.x * kRayDoubles + threadIdx.x] = block_total(s_w, threadIdx.x);
}

__global__ __launch_bounds__(256) void k_cmp_fit(CmpView v, CmpRot rot, double fit_radius) {
  __shared__ double s_w[4][16];
  double acc[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0}, used = 0.0, left = 0.0;
  const int base = blockIdx.x * kFitPerWg + threadIdx.x;
  for (int it = 0; it < kFitPerWg / 256; ++it) {                  // (ascending sample index within a lane)
    const int s = base + it * 256;
    if (s >= v.plan.n || v.flags0[s] != 0) continue;
    double qx, qy, rho;
    vc::cmp_sample(v.plan, s, &qx, &qy, &rho);
    if (!(rho <= fit_radius)) continue;
    const double* src = v.rays + 3 * (size_t)s;
    const double a[3] = {src[0], src[1], src[2]};
    if (vc::cmp_fit_sample(v.plan, rot.R, a, qx, qy, acc)) used += 1.0; else left += 1.0;
  }
#pragma unroll
  for (int k = 0; k < 10; ++k) block_stage(s_w, k, vc::wave_allsum(acc[k]));
  block_stage(s_w, 10, vc::wave_allsum(used));
  block_stage(s_w, 11, vc::wave_allsum(left));
  __syncthreads();
  if (threadIdx.x < vc::kCmpFitDoubles) v.part[(size_t)blockIdx.x * vc::kCmpFitDoubles + threadIdx.x] = block_total(s_w, threadIdx.x);
}

__global__ __launch_bounds__(256) void k_cmp_diff(CmpView v, CmpRot rot, int n_rings, int rings_only) {
  __shared__ double s_w[4][16];
  __shared__ double s_sq[256];          // |d|^2 of a valid sample, -1 of an invalid one
  __shared__ int s_ring[256];           // -1: no sample
  const int s = blockIdx.x * 256 + threadIdx.x;
  const double nan = __builtin_nan("");
  bool in = s < v.plan.n, valid = false;
  double du = 0.0, dv = 0.0;
  int ring = -1;
  if (in) {
    double qx, qy, rho;
    vc::cmp_sample(v.plan, s, &qx, &qy, &rho);
    ring = vc::cmp_ring(rho, n_rings);
    if (rings_only) {
      const double2 d = v.diff[s];
      valid = (v.flags[s] & vc::kCmpFlagInvalid) == 0;
      du = d.x; dv = d.y;
    } else {
      const int f0 = v.flags0[s];
      double d[2] = {nan, nan};
      if (f0 == 0) {
        const double* src = v.rays + 3 * (size_t)s;
        const double a[3] = {src[0], src[1], src[2]};
        valid = vc::cmp_diff_sample(v.plan, rot.R, a, qx, qy, d);
      }
      du = d[0]; dv = d[1];
      v.diff[s] = valid ? make_double2(du, dv) : make_double2(nan, nan);
      v.flags[s] = (unsigned char)(f0 | (valid ? 0 : vc::kCmpFlagInvalid));
    }
  }
  if (!valid) { du = 0.0; dv = 0.0; }
  const double sq = vc::cmp_norm2(du, dv);
  s_sq[threadIdx.x] = valid ? sq : -1.0;
  s_ring[threadIdx.x] = ring;
  // ---- the summary: sums by the butterfly; the maximum keeps the lower sample on ties
  const double cnt = vc::wave_allsum(valid ? 1.0 : 0.0), inv = vc::wave_allsum(in && !valid ? 1.0 : 0.0);
  const double s_du = vc::wave_allsum(du), s_dv = vc::wave_allsum(dv), s_q = vc::wave_allsum(sq);
  double best = valid ? sq : -1.0;
  int best_i = valid ? s : -1;
  vc::wave_argmax_low(&best, &best_i);
  block_stage(s_w, 0, cnt); block_stage(s_w, 1, inv); block_stage(s_w, 2, s_du); block_stage(s_w, 3, s_dv); block_stage(s_w, 4, s_q);
  block_stage(s_w, 5, best); block_stage(s_w, 6, (double)best_i);
  __syncthreads();
  double* rec = v.part + (size_t)blockIdx.x * kDiffDoubles;
  if (threadIdx.x < 5) rec[threadIdx.x] = block_total(s_w, threadIdx.x);
  if (threadIdx.x == 5) {                                          // waves hold ascending samples: a later wave wins only when larger
    double b = s_w[0][5], bi = s_w[0][6];
#pragma unroll
    for (int w = 1; w < 4; ++w) if (s_w[w][5] > b) { b = s_w[w][5]; bi = s_w[w][6]; }
    rec[5] = b; rec[6] = bi;
  }
  // ---- the rings: thread k owns ring k and walks the workgroup's entries in thread order
  if ((int)threadIdx.x < n_rings) {
    double rc = 0.0, ri = 0.0, rs = 0.0, rm = -1.0;
    for (int j = 0; j < 256; ++j) {
      if (s_ring[j] != (int)threadIdx.x) continue;
      const double q = s_sq[j];
      if (q >= 0.0) { rc += 1.0; rs += q; rm = q > rm ? q : rm; } else ri += 1.0;
    }
    double* r = rec + vc::kCmpSumDoubles + vc::kCmpRingDoubles * threadIdx.x;
    r[0] = rc; r[1] = ri; r[2] = rs; r[3] = rm;
  }
}

// columns of n_wg records of `stride` doubles added in workgroup order.  kReduceDiff: column 5 is a maximum that carries column 6 (its sample;
// strictly larger wins: workgroups hold ascending samples), every fourth ring column is a maximum.
__global__ __launch_bounds__(64) void k_cmp_reduce(const double* __restrict__ part, int n_wg, int stride, int m, int kind, double* __restrict__ out) {
  for (int c = threadIdx.x; c < m; c += 64) {
    const bool is_worst = kind == kReduceDiff && c == 5, is_idx = kind == kReduceDiff && c == 6;
    const bool is_max = kind == kReduceDiff && c >= vc::kCmpSumDoubles && ((c - vc::kCmpSumDoubles) & 3) == 3;
    if (is_idx) continue;                                          // (written with column 5)
    if (is_worst) {
      double b = -1.0, bi = -1.0;
      for (int g = 0; g < n_wg; ++g) {
        const double x = part[(size_t)g * stride + 5];
        if (x > b) { b = x; bi = part[(size_t)g * stride + 6]; }
      }
      out[5] = b; out[6] = bi;
    } else if (is_max) {
      double b = -1.0;
      for (int g = 0; g < n_wg; ++g) { const double x = part[(size_t)g * stride + c]; b = x > b ? x : b; }
      out[c] = b;
    } else {
      double t = 0.0;
      for (int g = 0; g < n_wg; ++g) t += part[(size_t)g * stride + c];
      out[c] = t;
    }
  }
}

}  // namespace

struct vc_comparer {
  int device = 0;
  CmpView v;
  hipStream_t stream = nullptr;
  unsigned char* d_buf = nullptr;      // [rays | diff | flags0 | flags | part | out]
  double* h_res = nullptr;             // pinned: the reduced record of the sweep in flight
  bool have_rays = false, have_run = false, in_flight = false;
  double rays_radius = 0.0;            // the fit radius H was summed for
  double H[9];
  long long n_fit = 0;
  double fit_radius = 0.0;             // the last run's
  vc::CmpFit fit;
  double summary[kDiffDoubles];        // the last run's, rings at kCmpDefaultRings
  int rings_n = 0;                     // ring count of `rings` (a rings-only sweep), 0 = none
  double rings[vc::kCmpRingDoubles * vc::kCmpMaxRings];
  int n_wg() const { return (v.plan.n + 255) / 256; }
  int n_wg_fit() const { return (v.plan.n + kFitPerWg - 1) / kFitPerWg; }
};

namespace {

void launch_rays(vc_comparer* c, double radius) {
  hipLaunchKernelGGL(k_cmp_rays, dim3(c->n_wg()), dim3(256), 0, c->stream, c->v, radius);
  hipLaunchKernelGGL(k_cmp_reduce, dim3(1), dim3(64), 0, c->stream, c->v.part, c->n_wg(), kRayDoubles, kRayDoubles, (int)kReduceSums, c->v.out);
}
void launch_fit(vc_comparer* c, const double* R, double radius) {
  CmpRot rot; std::memcpy(rot.R, R, 72);
  hipLaunchKernelGGL(k_cmp_fit, dim3(c->n_wg_fit()), dim3(256), 0, c->stream, c->v, rot, radius);
  hipLaunchKernelGGL(k_cmp_reduce, dim3(1), dim3(64), 0, c->stream, c->v.part, c->n_wg_fit(), (int)vc::kCmpFitDoubles, (int)vc::kCmpFitDoubles, (int)kReduceSums, c->v.out);
}
void launch_diff(vc_comparer* c, const double* R, int n_rings, int rings_only) {
  CmpRot rot; std::memcpy(rot.R, R, 72);
  hipLaunchKernelGGL(k_cmp_diff, dim3(c->n_wg()), dim3(256), 0, c->stream, c->v, rot, n_rings, rings_only);
  hipLaunchKernelGGL(k_cmp_reduce, dim3(1), dim3(64), 0, c->stream, c->v.part, c->n_wg(), kDiffDoubles, vc::kCmpSumDoubles + vc::kCmpRingDoubles * n_rings,
                     (int)kReduceDiff, c->v.out);
}
// the reduced record of what was just enqueued, in h_res: the one synchronisation of a sweep
bool fetch(vc_comparer* c, int m) {
  c->in_flight = true;
  if (hipGetLastError() != hipSuccess || hipMemcpyAsync(c->h_res, c->v.out, (size_t)m * 8, hipMemcpyDeviceToHost, c->stream) != hipSuccess ||
      hipStreamSynchronize(c->stream) != hipSuccess) return false;
  c->in_flight = false;
  return true;
}
bool grid_ok(int w, int h, int gx, int gy) { return gx >= 2 && gy >= 2 && gx <= w && gy <= h && (long long)gx * gy <= vc::kCmpMaxSamples; }

}  // namespace

extern "C" {

int vc_comparer_create(int device, int model_a, const double* params_a, int nparams_a, int model_b, const double* params_b, int nparams_b, int width, int height,
                       int grid_x, int grid_y, vc_comparer** out) {
  if (!out || !vc::undist_source_args_ok(model_a, params_a, nparams_a, width, height) || !vc::undist_source_args_ok(model_b, params_b, nparams_b, width, height) ||
      !grid_ok(width, height, grid_x, grid_y)) return VC_ERR_BAD_ARG;
  if (vch::open_device(device) != VC_OK) return VC_ERR_NO_DEVICE;
  vc_comparer* c = new vc_comparer;
  c->device = device;
  std::memset(&c->v, 0, sizeof(c->v)); std::memset(&c->fit, 0, sizeof(c->fit));
  CmpPlan& p = c->v.plan;
  p.model_a = model_a; p.model_b = model_b; p.w = width; p.h = height; p.gx = grid_x; p.gy = grid_y; p.n = grid_x * grid_y;
  for (int k = 0; k < nparams_a; ++k) p.Ka[k] = params_a[k];
  for (int k = 0; k < nparams_b; ++k) p.Kb[k] = params_b[k];
  vc::model_precompute(model_a, p.Ka, &p.pre_a); vc::model_precompute(model_b, p.Kb, &p.pre_b);
  auto carve = [&](vch::Carver q) {
    const size_t n = (size_t)p.n;
    c->v.rays = q.take<double>(n * 3);
    c->v.diff = q.take<double2>(n);
    c->v.flags0 = q.take<unsigned char>(n);
    c->v.flags = q.take<unsigned char>(n);
    c->v.part = q.take<double>((size_t)c->n_wg() * kDiffDoubles);
    c->v.out = q.take<double>(kDiffDoubles);
    return q.bytes();
  };
  if (hipStreamCreate(&c->stream) != hipSuccess || hipMalloc((void**)&c->d_buf, carve(vch::Carver())) != hipSuccess ||
      hipHostMalloc((void**)&c->h_res, kDiffDoubles * 8, hipHostMallocDefault) != hipSuccess) { vc_comparer_destroy(c); return VC_ERR_NO_DEVICE; }
  carve(vch::Carver(c->d_buf));
  *out = c;
  return VC_OK;
}
void vc_comparer_destroy(vc_comparer* c) {
  if (!c) return;
  (void)hipSetDevice(c->device);
  if (c->stream) { (void)hipStreamSynchronize(c->stream); (void)hipStreamDestroy(c->stream); }
  (void)hipFree(c->d_buf);
  if (c->h_res) (void)hipHostFree(c->h_res);
  delete c;
}

int vc_compare_run(vc_comparer* c, double fit_radius, int max_iters, const double R_ba[9]) {
  if (!c || !(fit_radius == fit_radius) || !(fit_radius <= 1e300)) return VC_ERR_BAD_ARG;
  const bool fitting = fit_radius > 0.0;
  double R0[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
  if (!fitting && R_ba) {
    if (!vc::is_rotation(R_ba)) return VC_ERR_BAD_ARG;
    std::memcpy(R0, R_ba, 72);
  }
  if (hipSetDevice(c->device) != hipSuccess) return VC_ERR_NO_DEVICE;
  if (c->in_flight) { (void)hipStreamSynchronize(c->stream); c->in_flight = false; }
  c->have_run = false; c->rings_n = 0;
  if (!c->have_rays || (fitting && fit_radius != c->rays_radius)) {
    c->have_rays = false;
    const double radius = fitting ? fit_radius : 0.0;
    launch_rays(c, radius);
    if (!fetch(c, kRayDoubles)) return VC_ERR_NO_DEVICE;
    std::memcpy(c->H, c->h_res, 72);
    c->n_fit = (long long)c->h_res[9];
    c->rays_radius = radius; c->have_rays = true;
  }
  vc::CmpFit& f = c->fit;
  std::memset(&f, 0, sizeof(f));
  if (fitting) {
    if (c->n_fit < 3) return VC_ERR_NUMERIC;
    vc::rigid_rotation(c->H, R0);
    const int rc = vc::cmp_gauss_newton([&](const double* R, double* sums) -> int {
      launch_fit(c, R, fit_radius);
      if (!fetch(c, vc::kCmpFitDoubles)) return (int)VC_ERR_NO_DEVICE;
      std::memcpy(sums, c->h_res, vc::kCmpFitDoubles * 8);
      return 0;
    }, R0, max_iters, &f);
    if (rc == -1) return VC_ERR_NUMERIC;
    if (rc != 0) return rc;
    f.n_fit = c->n_fit;
  } else {
    std::memcpy(f.R, R0, 72);
  }
  launch_diff(c, f.R, vc::kCmpDefaultRings, 0);
  if (!fetch(c, vc::kCmpSumDoubles + vc::kCmpRingDoubles * vc::kCmpDefaultRings)) return VC_ERR_NO_DEVICE;
  std::memcpy(c->summary, c->h_res, (vc::kCmpSumDoubles + vc::kCmpRingDoubles * vc::kCmpDefaultRings) * 8);
  c->fit_radius = fit_radius;
  c->have_run = true;
  return VC_OK;
}

int vc_compare_get_fit(vc_comparer* c, double R_ba[9], int* status, int* iterations, int* n_fit, int* n_left_out, double* cost0, double* cost) {
  if (!c || !c->have_run) return VC_ERR_BAD_ARG;
  const vc::CmpFit& f = c->fit;
  if (R_ba) std::memcpy(R_ba, f.R, 72);
  if (status) *status = f.status;
  if (iterations) *iterations = f.iterations;
  if (n_fit) *n_fit = (int)f.n_fit;
  if (n_left_out) *n_left_out = (int)f.n_left_out;
  if (cost0) *cost0 = f.cost0;
  if (cost) *cost = f.cost;
  return VC_OK;
}

int vc_compare_get_map(vc_comparer* c, double* diff, unsigned char* flags) {
  if (!c || !c->have_run) return VC_ERR_BAD_ARG;
  if (!diff && !flags) return VC_OK;
  if (hipSetDevice(c->device) != hipSuccess || hipStreamSynchronize(c->stream) != hipSuccess) return VC_ERR_NO_DEVICE;
  const size_t n = (size_t)c->v.plan.n;
  if (diff && hipMemcpy(diff, c->v.diff, n * 16, hipMemcpyDeviceToHost) != hipSuccess) return VC_ERR_NO_DEVICE;
  if (flags && hipMemcpy(flags, c->v.flags, n, hipMemcpyDeviceToHost) != hipSuccess) return VC_ERR_NO_DEVICE;
  return VC_OK;
}

int vc_compare_summary(vc_comparer* c, long long* count, long long* invalid, double* sum_du, double* sum_dv, double* sum_sq, double* max_err, long long* worst) {
  if (!c || !c->have_run) return VC_ERR_BAD_ARG;
  const double* s = c->summary;
  if (count) *count = (long long)s[0];
  if (invalid) *invalid = (long long)s[1];
  if (sum_du) *sum_du = s[2];
  if (sum_dv) *sum_dv = s[3];
  if (sum_sq) *sum_sq = s[4];
  if (max_err) *max_err = s[6] >= 0.0 ? std::sqrt(s[5]) : 0.0;      // (the host's square root of the largest |d|^2: monotone, so it is the largest |d|)
  if (worst) *worst = (long long)s[6];
  return VC_OK;
}

int vc_compare_rings(vc_comparer* c, int n_rings, long long* count, long long* invalid, double* sum_sq, double* max_err) {
  if (!c || !c->have_run || n_rings < 1 || n_rings > vc::kCmpMaxRings) return VC_ERR_BAD_ARG;
  const double* r = c->summary + vc::kCmpSumDoubles;
  if (n_rings != vc::kCmpDefaultRings) {
    if (c->rings_n != n_rings) {                                   // a rings-only sweep over the stored d: no inversion, no projection
      if (hipSetDevice(c->device) != hipSuccess) return VC_ERR_NO_DEVICE;
      c->rings_n = 0;
      launch_diff(c, c->fit.R, n_rings, 1);
      if (!fetch(c, vc::kCmpSumDoubles + vc::kCmpRingDoubles * n_rings)) return VC_ERR_NO_DEVICE;
      std::memcpy(c->rings, c->h_res + vc::kCmpSumDoubles, (size_t)vc::kCmpRingDoubles * n_rings * 8);
      c->rings_n = n_rings;
    }
    r = c->rings;
  }
  for (int k = 0; k < n_rings; ++k) {
    const double* q = r + vc::kCmpRingDoubles * k;
    if (count) count[k] = (long long)q[0];
    if (invalid) invalid[k] = (long long)q[1];
    if (sum_sq) sum_sq[k] = q[2];
    if (max_err) max_err[k] = q[0] > 0.0 ? std::sqrt(q[3]) : 0.0;
  }
  return VC_OK;
}

int vc_compare_extrinsics(const double T_ck_a0[7], const double T_ck_ac[7], const double T_ck_b0[7], const double T_ck_bc[7], const double R_0[9], const double R_c[9],
                          double out4[4]) {
  if (!out4) return VC_ERR_BAD_ARG;
  const double I[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
  double Tn[4][7];
  if (!vc::pose_ok(T_ck_a0, Tn[0]) || !vc::pose_ok(T_ck_ac, Tn[1]) || !vc::pose_ok(T_ck_b0, Tn[2]) || !vc::pose_ok(T_ck_bc, Tn[3])) return VC_ERR_BAD_ARG;
  if ((R_0 && !vc::is_rotation(R_0)) || (R_c && !vc::is_rotation(R_c))) return VC_ERR_BAD_ARG;
  vc::cmp_extrinsics(Tn[0], Tn[1], Tn[2], Tn[3], R_0 ? R_0 : I, R_c ? R_c : I, out4);
  vc::cmp_extrinsics(Tn[0], Tn[1], Tn[2], Tn[3], I, I, out4 + 2);
  return VC_OK;
}

int vc_time_compare(vc_comparer* c, int reps, double out_ms[3]) {
  if (!c || reps < 1 || !out_ms || !c->have_run) return VC_ERR_BAD_ARG;
  if (hipSetDevice(c->device) != hipSuccess) return VC_ERR_NO_DEVICE;
  if (c->in_flight) { (void)hipStreamSynchronize(c->stream); c->in_flight = false; }
  for (int what = 0; what < 3; ++what) {
    auto launch = [&]() {                                          // (each rewrites what the last run left: the same rays, the same map)
      if (what == 0) launch_rays(c, c->rays_radius);
      else if (what == 1) launch_fit(c, c->fit.R, c->fit_radius > 0.0 ? c->fit_radius : 1e300);
      else launch_diff(c, c->fit.R, vc::kCmpDefaultRings, 0);
    };
    const int rc = vch::time_back_to_back(c->stream, reps, launch, &out_ms[what]);
    if (rc != VC_OK) return rc;
  }
  return VC_OK;
}

}  // extern "C"
