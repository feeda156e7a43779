// vc_stereo_uncertainty.hip -- the row and depth uncertainty of a calibrated stereo pair mapped over its rectified image on the GPU (gfx950,
// wave64, fp64).  A vc_stereo_uncertainty holds cameras A and B, their rectified frames, the destination pinhole and a lattice of
// n = gx * gy samples (vc_stereo_uncertainty.hpp has the arithmetic).  Nothing is allocated beyond the handle's buffers and nothing is
// launched before the first vc_stereo_uncertainty_run.  Per depth plane, one after the other on the handle's stream:
//   k_su_side<MODEL>   one sample per thread, launched once per side: the point at depth Z, its ray in the camera, project_any<true>, the
//                      side's block [-Pi [r]x | Pi R_ds da/dK] padded to 2 x 13 and the side's flag stored -- column by column, so that a
//                      wave writes (and k_su_map reads) whole lines.  The only kernel that knows a camera model: one instantiation per
//                      model through with_model, and a sample pays for its two projections once, not once per row.
//   k_su_map           model-free, every size a compile-time constant: both blocks read, the rows of dv and d (27 each) formed in registers
//                      and put through the packed 27 x 27 Cov_eta in LDS in one pass (su_variances; every lane reads the same address: a
//                      broadcast), the triple (var_dv, var_d, var_Z) and the flags stored, then the workgroup's record (lat_block_record):
//                      count, invalid, the three sums, the largest var_dv and its sample (the lowest on ties).
//   k_lat_reduce       the workgroups' records folded into the plane's seven doubles of the handle's record.
// The block buffer and the workgroups' records are reused between planes (the stream orders them); one host synchronisation per run.  No
// floating-point atomic anywhere; the workgroup decomposition depends on n alone: two runs, and two handles, give the same bits, and a
// plane's bits do not depend on the planes beside it.  No CPU fallback: vc_stereo_uncertainty_create fails with VC_ERR_NO_DEVICE without a
// HIP device.  The record (lat_block_record), its fold (k_lat_reduce) and the handle's device side (LatticeHandle) are the lattice core's.
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstring>
#include <vector>
#include "../../include/vicalib_amd.h"
#include "vc_lattice.hpp"
#include "vc_stereo_uncertainty.hpp"

namespace {

using vc::SuCov;
using vc::SuPlan;

struct SuView {
  SuPlan plan;
  double* blk;                 // 2 x 26 x n, [side][column][sample]: the plane in flight
  unsigned char* sflag;        // 2 x n: 1 = the side has no block at this sample
  double* cov;                 // 378: sigma_px^2 Cov_eta, packed
  double* var;                 // planes x n x 3
  unsigned char* flags;        // planes x n
  double* part;                // one record per workgroup of the map sweep in flight
};

template <int MODEL>
__global__ __launch_bounds__(256) void k_su_side(SuView v, int side, double Z) {
  const int s = blockIdx.x * 256 + threadIdx.x, n = v.plan.lat.n;
  if (s >= n) return;
  double r[3], blk[vc::kSuSideDoubles];
  vc::su_point(v.plan, s, Z, side, r);
  const bool ok = side ? vc::su_side_block<MODEL>(v.plan.lat.Kb, v.plan.lat.pre_b, v.plan.src_w[1], v.plan.src_h[1], v.plan.R_ds[1], v.plan.dl, r, blk)
                       : vc::su_side_block<MODEL>(v.plan.lat.Ka, v.plan.lat.pre_a, v.plan.src_w[0], v.plan.src_h[0], v.plan.R_ds[0], v.plan.dl, r, blk);
  v.sflag[(size_t)side * n + s] = ok ? 0 : 1;
  if (!ok) return;
  double* dst = v.blk + (size_t)side * vc::kSuSideDoubles * n + s;
#pragma unroll
  for (int k = 0; k < vc::kSuSideDoubles; ++k) dst[(size_t)k * n] = blk[k];
}

__global__ __launch_bounds__(256) void k_su_map(SuView v, int plane, double Z) {
  __shared__ double s_P[vc::kSuPacked];
  for (int k = threadIdx.x; k < vc::kSuPacked; k += 256) s_P[k] = v.cov[k];
  __syncthreads();
  const int s = blockIdx.x * 256 + threadIdx.x, n = v.plan.lat.n;
  const double nan = __builtin_nan("");
  const bool in = s < n;
  bool valid = false;
  double var[3] = {0.0, 0.0, 0.0};
  if (in) {
    const int fa = v.sflag[s], fb = v.sflag[(size_t)n + s];
    if (fa == 0 && fb == 0) {
      double ba[vc::kSuSideDoubles], bb[vc::kSuSideDoubles];
      const double* src = v.blk + s;
#pragma unroll
      for (int k = 0; k < vc::kSuSideDoubles; ++k) { ba[k] = src[(size_t)k * n]; bb[k] = src[(size_t)(vc::kSuSideDoubles + k) * n]; }
      valid = vc::su_variances(ba, bb, v.plan.dl[0], Z, v.plan.baseline, s_P, var);
    }
    double* dst = v.var + ((size_t)plane * n + s) * 3;
    dst[0] = valid ? var[0] : nan; dst[1] = valid ? var[1] : nan; dst[2] = valid ? var[2] : nan;
    v.flags[(size_t)plane * n + s] = (unsigned char)((fa ? vc::kCmpFlagA : 0) | (fb ? vc::kCmpFlagB : 0) | (valid ? 0 : vc::kCmpFlagInvalid));
  }
  if (!valid) { var[0] = 0.0; var[1] = 0.0; var[2] = 0.0; }
  const double sums[5] = {valid ? 1.0 : 0.0, in && !valid ? 1.0 : 0.0, var[0], var[1], var[2]};
  vc::lat_block_record<5, true>(v.part + (size_t)blockIdx.x * vc::kSuSumDoubles, sums, valid ? var[0] : -1.0, valid ? s : -1);
}

}  // namespace

struct vc_stereo_uncertainty : vc::LatticeHandle {   // d_buf: [blk | var | cov | sflag | flags | part]
  SuView v;
  int nk[2] = {0, 0};
  double T_ck[2][7];                   // normalised
  double W[84];                        // rect_pose_jacobian
  bool have_run = false, have_cal_cov = false;
  double cal_cov[vc::kSuMaxCov * vc::kSuMaxCov];       // the calibrator's (vc_stereo_uncertainty_create_for_cameras)
  SuCov cov;                           // the last run's
  int n_depths = 0;
  double depths[vc::kSuMaxDepths];
  double summary[vc::kSuSumDoubles * vc::kSuMaxDepths];
  int n_cov() const { return 14 + nk[0] + nk[1]; }
  int n_wg() const { return (v.plan.lat.n + 255) / 256; }
};

namespace {

void launch_sides(vc_stereo_uncertainty* u, double Z) {
  for (int side = 0; side < 2; ++side)
    vc::with_model(side ? u->v.plan.lat.model_b : u->v.plan.lat.model_a, [&](auto m) {
      hipLaunchKernelGGL(k_su_side<decltype(m)::value>, dim3(u->n_wg()), dim3(256), 0, u->stream, u->v, side, Z);
    });
}
void launch_map(vc_stereo_uncertainty* u, int plane, double Z) {
  hipLaunchKernelGGL(k_su_map, dim3(u->n_wg()), dim3(256), 0, u->stream, u->v, plane, Z);
  hipLaunchKernelGGL(k_lat_reduce<true>, dim3(1), dim3(64), 0, u->stream, (const double*)u->v.part, u->n_wg(), vc::kSuSumDoubles, vc::kSuSumDoubles,
                     vc::kSuSumDoubles - 2, vc::kLatNone, u->d_res + (size_t)plane * vc::kSuSumDoubles);
}

}  // namespace

void vc::su_attach_cov(vc_stereo_uncertainty* u, const double* cov) {
  std::memcpy(u->cal_cov, cov, (size_t)u->n_cov() * u->n_cov() * 8);
  u->have_cal_cov = true;
}

extern "C" {

int vc_stereo_pose_jacobian(const double T_ck_a[7], const double T_ck_b[7], double W[84]) {
  double Ta[7], Tb[7];
  if (!W || !vc::pose_ok(T_ck_a, Ta) || !vc::pose_ok(T_ck_b, Tb)) return VC_ERR_BAD_ARG;
  const int rc = vc::rect_pose_jacobian(Ta, Tb, W);
  return rc == vc::kRectOk ? VC_OK : rc == vc::kRectCoincident ? VC_ERR_NUMERIC : VC_ERR_UNSUPPORTED;
}

int vc_stereo_uncertainty_create(int device, int model_a, const double* params_a, int nparams_a, int w_a, int h_a, const double T_ck_a[7], int model_b,
                                 const double* params_b, int nparams_b, int w_b, int h_b, const double T_ck_b[7], const double dst_linear[4], int dst_w, int dst_h,
                                 double alpha, int grid_x, int grid_y, vc_stereo_uncertainty** out) {
  double Ta[7], Tb[7];
  if (!out || !vc::undist_source_args_ok(model_a, params_a, nparams_a, w_a, h_a) || !vc::undist_source_args_ok(model_b, params_b, nparams_b, w_b, h_b)) return VC_ERR_BAD_ARG;
  if (!vc::undist_dest_args_ok(dst_linear, dst_w, dst_h, 0) || !vc::pose_ok(T_ck_a, Ta) || !vc::pose_ok(T_ck_b, Tb)) return VC_ERR_BAD_ARG;
  if ((!dst_linear && !(alpha >= 0.0 && alpha <= 1.0)) || !vc::cvt_grid_ok(dst_w, dst_h, grid_x, grid_y)) return VC_ERR_BAD_ARG;
  vc_stereo_uncertainty* u = new vc_stereo_uncertainty;
  std::memset(&u->v, 0, sizeof(u->v)); std::memset(&u->cov, 0, sizeof(u->cov));
  SuPlan& p = u->v.plan;
  int rc = vc_stereo_rectify_rotations(Ta, Tb, p.R_ds[0], p.R_ds[1], &p.baseline);
  if (rc == VC_OK) rc = vc_stereo_pose_jacobian(Ta, Tb, u->W);
  if (rc == VC_OK) {
    if (dst_linear) std::memcpy(p.dl, dst_linear, 32);
    else rc = vc_stereo_fit_linear(model_a, params_a, nparams_a, w_a, h_a, p.R_ds[0], model_b, params_b, nparams_b, w_b, h_b, p.R_ds[1], dst_w, dst_h, alpha, p.dl);
  }
  if (rc != VC_OK) { delete u; return rc; }
  vc::cmp_plan_set(&p.lat, model_a, params_a, nparams_a, model_b, params_b, nparams_b, dst_w, dst_h, grid_x, grid_y);      // (only p.lat is reset)
  p.src_w[0] = w_a; p.src_h[0] = h_a; p.src_w[1] = w_b; p.src_h[1] = h_b;
  u->nk[0] = nparams_a; u->nk[1] = nparams_b;
  std::memcpy(u->T_ck[0], Ta, 56); std::memcpy(u->T_ck[1], Tb, 56);
  auto carve = [&](vch::Carver q) {
    const size_t n = (size_t)p.lat.n;
    u->v.blk = q.take<double>(n * 2 * vc::kSuSideDoubles);
    u->v.var = q.take<double>(n * 3 * vc::kSuMaxDepths);
    u->v.cov = q.take<double>(vc::kSuPacked);
    u->v.sflag = q.take<unsigned char>(n * 2);
    u->v.flags = q.take<unsigned char>(n * vc::kSuMaxDepths);
    u->v.part = q.take<double>((size_t)u->n_wg() * vc::kSuSumDoubles);
    return q.bytes();
  };
  if (!u->open(device, carve(vch::Carver()), vc::kSuSumDoubles * vc::kSuMaxDepths)) { delete u; return VC_ERR_NO_DEVICE; }
  carve(vch::Carver(u->d_buf));
  *out = u;
  return VC_OK;
}
void vc_stereo_uncertainty_destroy(vc_stereo_uncertainty* u) {
  if (!u) return;
  u->close();
  delete u;
}

int vc_stereo_uncertainty_get(vc_stereo_uncertainty* u, double R_ds_a[9], double R_ds_b[9], double dst_linear[4], double* baseline, double W[84]) {
  if (!u) return VC_ERR_BAD_ARG;
  if (R_ds_a) std::memcpy(R_ds_a, u->v.plan.R_ds[0], 72);
  if (R_ds_b) std::memcpy(R_ds_b, u->v.plan.R_ds[1], 72);
  if (dst_linear) std::memcpy(dst_linear, u->v.plan.dl, 32);
  if (baseline) *baseline = u->v.plan.baseline;
  if (W) std::memcpy(W, u->W, sizeof(u->W));
  return VC_OK;
}

int vc_stereo_uncertainty_run(vc_stereo_uncertainty* u, const double* cov, double sigma_px, const double* depths, int n_depths) {
  if (!u) return VC_ERR_BAD_ARG;
  u->have_run = false;                                             // a refused run leaves nothing to read
  if (!cov && !u->have_cal_cov) return VC_ERR_BAD_ARG;
  const double* c = cov ? cov : u->cal_cov;
  const int n = u->n_cov();
  if (!vc::su_run_args_ok(c, n, sigma_px, depths, n_depths)) return VC_ERR_BAD_ARG;
  if (!u->settle()) return VC_ERR_NO_DEVICE;
  double T[vc::kSuEta * vc::kSuMaxCov];
  vc::su_eta_map(u->T_ck[0], u->T_ck[1], u->nk[0], u->nk[1], u->W, T);
  vc::su_pack_cov(c, n, T, sigma_px, &u->cov);
  if (hipMemcpyAsync(u->v.cov, u->cov.P, sizeof(u->cov.P), hipMemcpyHostToDevice, u->stream) != hipSuccess) return VC_ERR_NO_DEVICE;
  for (int k = 0; k < n_depths; ++k) {
    launch_sides(u, depths[k]);
    launch_map(u, k, depths[k]);
  }
  if (!u->fetch(vc::kSuSumDoubles * n_depths)) return VC_ERR_NO_DEVICE;
  std::memcpy(u->summary, u->h_res, (size_t)vc::kSuSumDoubles * n_depths * 8);
  std::memcpy(u->depths, depths, (size_t)n_depths * 8);
  u->n_depths = n_depths;
  u->have_run = true;
  return VC_OK;
}

int vc_stereo_uncertainty_get_map(vc_stereo_uncertainty* u, double* var, unsigned char* flags) {
  if (!u || !u->have_run) return VC_ERR_BAD_ARG;
  if (!var && !flags) return VC_OK;
  if (hipSetDevice(u->device) != hipSuccess || hipStreamSynchronize(u->stream) != hipSuccess) return VC_ERR_NO_DEVICE;
  const size_t n = (size_t)u->v.plan.lat.n * u->n_depths;
  if (var && hipMemcpy(var, u->v.var, n * 24, hipMemcpyDeviceToHost) != hipSuccess) return VC_ERR_NO_DEVICE;
  if (flags && hipMemcpy(flags, u->v.flags, n, hipMemcpyDeviceToHost) != hipSuccess) return VC_ERR_NO_DEVICE;
  return VC_OK;
}

int vc_stereo_uncertainty_summary(vc_stereo_uncertainty* u, int plane, long long* count, long long* invalid, double* sum_var_dv, double* sum_var_d, double* sum_var_z,
                                  double* max_var_dv, long long* worst) {
  if (!u || !u->have_run || plane < 0 || plane >= u->n_depths) return VC_ERR_BAD_ARG;
  const double* s = u->summary + (size_t)plane * vc::kSuSumDoubles;
  if (count) *count = (long long)s[0];
  if (invalid) *invalid = (long long)s[1];
  if (sum_var_dv) *sum_var_dv = s[2];
  if (sum_var_d) *sum_var_d = s[3];
  if (sum_var_z) *sum_var_z = s[4];
  if (max_var_dv) *max_var_dv = s[6] >= 0.0 ? s[5] : 0.0;
  if (worst) *worst = (long long)s[6];
  return VC_OK;
}

int vc_stereo_uncertainty_get_pose_sigma(vc_stereo_uncertainty* u, double var[7]) {
  if (!u || !u->have_run || !var) return VC_ERR_BAD_ARG;
  for (int k = 0; k < 7; ++k) var[k] = u->cov.P[vc::su_pidx(k, k)];
  return VC_OK;
}

int vc_time_stereo_uncertainty(vc_stereo_uncertainty* u, int reps, double out_ms[2]) {
  if (!u || reps < 1 || !out_ms || !u->have_run) return VC_ERR_BAD_ARG;
  if (!u->settle()) return VC_ERR_NO_DEVICE;
  const int last = u->n_depths - 1;                                // (each rewrites what the last run left: the last plane's blocks, its map)
  for (int what = 0; what < 2; ++what) {
    auto launch = [&]() {
      if (what == 0) launch_sides(u, u->depths[last]);
      else launch_map(u, last, u->depths[last]);
    };
    const int rc = vch::time_back_to_back(u->stream, reps, launch, &out_ms[what]);
    if (rc != VC_OK) return rc;
  }
  return VC_OK;
}

}  // extern "C"
