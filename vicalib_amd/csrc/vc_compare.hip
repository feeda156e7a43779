// vc_compare.hip -- two calibrations of one camera compared in pixel space on the GPU (gfx950, wave64, fp64).
//
// A vc_comparer holds cameras A and B of one image size and a lattice of n = gx * gy samples (vc_compare.hpp has the arithmetic).  Nothing is
// allocated beyond the handle's buffers and nothing is launched before the first vc_compare_run.
//
//   k_cmp_rays    one sample per thread: both Newton inversions (undist_unproject), the unit ray a stored, the inversion flags, and the
//                 workgroup's partial of Horn's H = sum over the fit set of a b^T with the size of the fit set.  It runs once per handle and
//                 again only when a run asks for another fit radius (the fit set is part of H).
//   k_cmp_fit     one Gauss-Newton evaluation at a rotation R: 1024 samples per 256-thread workgroup, a lane takes its four samples in index
//                 order and keeps J^T J (6), J^T d (3), E and the two counts in registers.
//   k_cmp_diff    the difference sweep at the final R, one sample per thread: d and the flags stored, the workgroup's partial of the summary
//                 and of the rings, for which every thread leaves its ring and |d|^2 in LDS.  With rings_only it reads the stored d instead
//                 of computing it: vc_compare_rings at another ring count inverts and projects nothing.
// The workgroup's record (lat_block_record), the rings (lat_ring_walk), the fold of the records (k_lat_reduce) and the handle's device side
// (LatticeHandle) are the lattice core's, vc_lattice.hpp, shared with the converter and the uncertainty map.
// No floating-point atomic anywhere; the workgroup decomposition depends on n alone: two runs, and two handles, give the same bits.
// One host synchronisation per Gauss-Newton evaluation and one for the difference sweep.  No CPU fallback: vc_comparer_create fails with
// VC_ERR_NO_DEVICE without a HIP device.  vc_compare_extrinsics is host code and needs none.
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstring>
#include <vector>
#include "../../include/vicalib_amd.h"
#include "vc_lattice.hpp"

namespace {

using vc::CmpPlan;
constexpr int kFitPerWg = 1024;
constexpr int kRayDoubles = 10;                                                       // H (9), size of the fit set
constexpr int kDiffDoubles = vc::kCmpSumDoubles + vc::kCmpRingDoubles * vc::kCmpMaxRings;   // a workgroup's record of the difference sweep
static_assert(vc::kCmpRingDoubles == vc::kLatRingDoubles, "a ring's record is the lattice core's");

struct CmpView {
  CmpPlan plan;
  double* rays;                // n x 3: a
  unsigned char* flags0;       // n: bits 0 and 1, as k_cmp_rays left them
  unsigned char* flags;        // n: the last difference sweep's, bit 2 added
  double2* diff;               // n
  double* part;                // workgroup partials of the kernel in flight
};
struct CmpRot { double R[9]; };

__global__ __launch_bounds__(256) void k_cmp_rays(CmpView v, double fit_radius) {
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
  const double sums[kRayDoubles] = {H[0], H[1], H[2], H[3], H[4], H[5], H[6], H[7], H[8], nf};
  vc::lat_block_record(v.part + (size_t)blockIdx.x * kRayDoubles, sums);
}

__global__ __launch_bounds__(256) void k_cmp_fit(CmpView v, CmpRot rot, double fit_radius) {
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
  const double sums[vc::kCmpFitDoubles] = {acc[0], acc[1], acc[2], acc[3], acc[4], acc[5], acc[6], acc[7], acc[8], acc[9], used, left};
  vc::lat_block_record(v.part + (size_t)blockIdx.x * vc::kCmpFitDoubles, sums);
}

__global__ __launch_bounds__(256) void k_cmp_diff(CmpView v, CmpRot rot, int n_rings, int rings_only) {
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
  // the summary (count, invalid, sum du, sum dv, sum |d|^2, the largest |d|^2 and its sample), then the rings: |d|^2 is summed and is the key
  double* rec = v.part + (size_t)blockIdx.x * kDiffDoubles;
  const double sums[5] = {valid ? 1.0 : 0.0, in && !valid ? 1.0 : 0.0, du, dv, sq};
  vc::lat_block_record<5, true>(rec, sums, valid ? sq : -1.0, valid ? s : -1);
  vc::lat_ring_walk(rec + vc::kCmpSumDoubles, n_rings, s_ring, s_sq, s_sq);
}

}  // namespace

struct vc_comparer : vc::LatticeHandle {      // d_buf: [rays | diff | flags0 | flags | part]
  CmpView v;
  bool have_rays = false, have_run = false;
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
  c->reduce(c->v.part, c->n_wg(), kRayDoubles, kRayDoubles);
}
void launch_fit(vc_comparer* c, const double* R, double radius) {
  CmpRot rot; std::memcpy(rot.R, R, 72);
  hipLaunchKernelGGL(k_cmp_fit, dim3(c->n_wg_fit()), dim3(256), 0, c->stream, c->v, rot, radius);
  c->reduce(c->v.part, c->n_wg_fit(), vc::kCmpFitDoubles, vc::kCmpFitDoubles);
}
void launch_diff(vc_comparer* c, const double* R, int n_rings, int rings_only) {
  CmpRot rot; std::memcpy(rot.R, R, 72);
  hipLaunchKernelGGL(k_cmp_diff, dim3(c->n_wg()), dim3(256), 0, c->stream, c->v, rot, n_rings, rings_only);
  c->reduce(c->v.part, c->n_wg(), kDiffDoubles, vc::kCmpSumDoubles + vc::kCmpRingDoubles * n_rings, vc::kCmpSumDoubles - 2, vc::kCmpSumDoubles);
}

}  // namespace

extern "C" {

int vc_comparer_create(int device, int model_a, const double* params_a, int nparams_a, int model_b, const double* params_b, int nparams_b, int width, int height,
                       int grid_x, int grid_y, vc_comparer** out) {
  if (!out || !vc::undist_source_args_ok(model_a, params_a, nparams_a, width, height) || !vc::undist_source_args_ok(model_b, params_b, nparams_b, width, height) ||
      !vc::cvt_grid_ok(width, height, grid_x, grid_y)) return VC_ERR_BAD_ARG;
  vc_comparer* c = new vc_comparer;
  std::memset(&c->v, 0, sizeof(c->v)); std::memset(&c->fit, 0, sizeof(c->fit));
  vc::cmp_plan_set(&c->v.plan, model_a, params_a, nparams_a, model_b, params_b, nparams_b, width, height, grid_x, grid_y);
  auto carve = [&](vch::Carver q) {
    const size_t n = (size_t)c->v.plan.n;
    c->v.rays = q.take<double>(n * 3);
    c->v.diff = q.take<double2>(n);
    c->v.flags0 = q.take<unsigned char>(n);
    c->v.flags = q.take<unsigned char>(n);
    c->v.part = q.take<double>((size_t)c->n_wg() * kDiffDoubles);
    return q.bytes();
  };
  if (!c->open(device, carve(vch::Carver()), kDiffDoubles)) { delete c; return VC_ERR_NO_DEVICE; }
  carve(vch::Carver(c->d_buf));
  *out = c;
  return VC_OK;
}
void vc_comparer_destroy(vc_comparer* c) {
  if (!c) return;
  c->close();
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
  if (!c->settle()) return VC_ERR_NO_DEVICE;
  c->have_run = false; c->rings_n = 0;
  if (!c->have_rays || (fitting && fit_radius != c->rays_radius)) {
    c->have_rays = false;
    const double radius = fitting ? fit_radius : 0.0;
    launch_rays(c, radius);
    if (!c->fetch(kRayDoubles)) return VC_ERR_NO_DEVICE;
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
      if (!c->fetch(vc::kCmpFitDoubles)) return (int)VC_ERR_NO_DEVICE;
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
  if (!c->fetch(vc::kCmpSumDoubles + vc::kCmpRingDoubles * vc::kCmpDefaultRings)) return VC_ERR_NO_DEVICE;
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
      if (!c->fetch(vc::kCmpSumDoubles + vc::kCmpRingDoubles * n_rings)) return VC_ERR_NO_DEVICE;
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
  if (!c->settle()) return VC_ERR_NO_DEVICE;
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
