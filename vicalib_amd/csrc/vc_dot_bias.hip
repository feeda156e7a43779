// vc_dot_bias.hip -- the predicted centre bias of every dot observation of a calibration at once (gfx950, wave64, fp64 throughout):
// vc_dot_bias_batch.  vc_dot_bias.hpp has the arithmetic, vc_conic5.hpp the 5 x 5 solve it shares with the detector.
//
//  k_dot_bias   one wavefront per observation, four observations per workgroup, NO BLOCK BARRIER and no LDS.  Lane i holds boundary sample i
//               of the dot's rim: its projection with the Jacobian, its edge line and its twenty products stay in that lane's registers; the
//               twenty sums are the fixed-order xor butterfly (wave_allsum), after which every lane holds the same normal equations and
//               solves them (vc_conic5.hpp: selects, no array indexed at run time).  The observation and its view are wave-uniform
//               (readfirstlane): model, intrinsics and pose of the view come by scalar loads through the scalar cache the waves of a
//               compute unit share, and the observations of a view are neighbours in the batch, so the waves of a workgroup read the same
//               model id and 17 doubles.  Every branch behind the centre's test and behind a sum is wave-uniform; lane 0 writes the result.
//               An observation gives the same bits alone, among others and on a second run: nothing in it depends on its place in the batch.
// No floating-point atomic.  No CPU fallback: without a device the entry point fails.
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstring>
#include <vector>
#include "../../include/vicalib_amd.h"
#include "vc_kutil.hpp"
#include "vc_hostutil.hpp"
#include "vc_dot_bias.hpp"

namespace {

struct DotBiasBatch {
  int total;
  const int* __restrict__ model;       // per view
  const double* __restrict__ K;        // per view x 10
  const double* __restrict__ T;        // per view x 7
  const int* __restrict__ obs_view;    // per observation: its view
  const double* __restrict__ pw;       // total x 3
  const double* __restrict__ radius;   // total
  double* __restrict__ bias;           // total x 2
  double* __restrict__ radius_px;      // total
  int* __restrict__ status;            // total
};

// the observation's 64 lanes (vc_seed.hpp: W)
struct DotBiasWave {
  static constexpr int kLanes = 64;
  int lane;
  __device__ __forceinline__ double allsum(double x) const { return vc::wave_allsum(x); }
  __device__ __forceinline__ int allsum(int x) const { return vc::wave_allsum(x); }
};

__global__ __launch_bounds__(256) void k_dot_bias(DotBiasBatch b) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int o = __builtin_amdgcn_readfirstlane(blockIdx.x * 4 + wave);      // (scalar: the observation, its view and the view's camera are loaded once per wave)
  if (o >= b.total) return;                                        // (a whole wave leaves: nothing in this kernel waits for another wave)
  const int v = __builtin_amdgcn_readfirstlane(b.obs_view[o]);
  vc::DotBiasView view;
  vc::dot_bias_view(b.model[v], b.K + (size_t)v * 10, b.T + (size_t)v * 7, &view);
  const double C[3] = {b.pw[3 * (size_t)o], b.pw[3 * (size_t)o + 1], b.pw[3 * (size_t)o + 2]};
  double bias[2] = {0.0, 0.0}, radius_px = 0.0;
  const int status = vc::dot_bias_one(DotBiasWave{lane}, view, C, b.radius[o], bias, &radius_px);
  if (lane == 0) {
    b.status[o] = status;
    if (status == vc::kDotBiasOk) { b.bias[2 * (size_t)o] = bias[0]; b.bias[2 * (size_t)o + 1] = bias[1]; b.radius_px[o] = radius_px; }
  }
}

}  // namespace

namespace vc {

bool dot_bias_args_ok(int n_views, const int* view_model, const double* view_K, const double* view_T_cw, const int* view_off, const double* p_w,
                      const double* radius, const double* bias, const double* radius_px, const int* status) {
  if (n_views < 0 || !view_model || !view_K || !view_T_cw || !view_off || !p_w || !radius || !bias || !radius_px || !status) return false;
  if (view_off[0] < 0) return false;
  for (int v = 0; v < n_views; ++v)
    if (view_off[v + 1] < view_off[v] || model_nk(view_model[v]) < 0) return false;
  for (int i = view_off[0]; i < view_off[n_views]; ++i)
    if (!(radius[i] >= 0.0) || !seed_finite(radius[i])) return false;
  return true;
}

int dot_bias_run(int device, int n_views, const int* view_model, const double* view_K, const double* view_T_cw, const int* view_off, const double* p_w,
                 const double* radius, double* bias, double* radius_px, int* status, int time_reps, double* kernel_ms) {
  if (kernel_ms) *kernel_ms = 0.0;
  if (vch::open_device(device) != VC_OK) return VC_ERR_NO_DEVICE;
  const size_t first = (size_t)view_off[0], total = (size_t)view_off[n_views] - first, nv = (size_t)n_views;
  if (total == 0) return VC_OK;
  hipStream_t stream = nullptr;
  std::vector<int> obs_view(total);
  for (size_t v = 0; v < nv; ++v)
    for (int i = view_off[v]; i < view_off[v + 1]; ++i) obs_view[(size_t)i - first] = (int)v;
  DotBiasBatch b;
  std::memset(&b, 0, sizeof(b));
  b.total = (int)total;
  int *d_model = nullptr, *d_obs_view = nullptr, *d_status = nullptr;
  double *d_K = nullptr, *d_T = nullptr, *d_pw = nullptr, *d_radius = nullptr, *d_bias = nullptr, *d_radius_px = nullptr;
  auto carve = [&](vch::Carver q) {
    d_model = q.take<int>(nv); d_K = q.take<double>(nv * 10); d_T = q.take<double>(nv * 7); d_obs_view = q.take<int>(total);
    d_pw = q.take<double>(3 * total); d_radius = q.take<double>(total);
    d_bias = q.take<double>(2 * total); d_radius_px = q.take<double>(total); d_status = q.take<int>(total);
    return q.bytes();
  };
  unsigned char* d_buf = nullptr;
  if (hipMalloc((void**)&d_buf, carve(vch::Carver())) != hipSuccess) return VC_ERR_NO_DEVICE;
  carve(vch::Carver(d_buf));
  b.model = d_model; b.K = d_K; b.T = d_T; b.obs_view = d_obs_view; b.pw = d_pw; b.radius = d_radius;
  b.bias = d_bias; b.radius_px = d_radius_px; b.status = d_status;
  std::vector<double> h_bias(2 * total), h_radius_px(total);
  auto up = [&](void* dst, const void* src, size_t bytes) { return bytes == 0 || hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, stream) == hipSuccess; };
  auto down = [&](void* dst, const void* src, size_t bytes) { return bytes == 0 || hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, stream) == hipSuccess; };
  auto launch = [&]() { hipLaunchKernelGGL(k_dot_bias, dim3((unsigned)((total + 3) / 4)), dim3(256), 0, stream, b); };
  bool ok = up(d_model, view_model, nv * 4) && up(d_K, view_K, nv * 80) && up(d_T, view_T_cw, nv * 56) && up(d_obs_view, obs_view.data(), total * 4) &&
            up(d_pw, p_w + 3 * first, total * 24) && up(d_radius, radius + first, total * 8);
  if (ok) {
    launch();
    ok = hipGetLastError() == hipSuccess && down(h_bias.data(), d_bias, total * 16) && down(h_radius_px.data(), d_radius_px, total * 8) &&
         down(status + first, d_status, total * 4);
  }
  ok = hipStreamSynchronize(stream) == hipSuccess && ok;
  if (ok && kernel_ms && time_reps > 0)                              // (the kernel again on the same input: it writes the same bits)
    ok = vch::time_back_to_back(stream, time_reps, launch, kernel_ms) == VC_OK;
  (void)hipFree(d_buf);
  if (!ok) return VC_ERR_NO_DEVICE;
  for (size_t i = 0; i < total; ++i) {                               // a refused observation's outputs are the caller's, untouched
    if (status[first + i] != kDotBiasOk) continue;
    bias[2 * (first + i)] = h_bias[2 * i]; bias[2 * (first + i) + 1] = h_bias[2 * i + 1];
    radius_px[first + i] = h_radius_px[i];
  }
  return VC_OK;
}

}  // namespace vc

extern "C" int vc_dot_bias_batch(int device, int n_views, const int* view_model, const double* view_K, const double* view_T_cw, const int* view_off,
                                 const double* p_w, const double* radius, double* bias, double* radius_px, int* status) {
  if (!vc::dot_bias_args_ok(n_views, view_model, view_K, view_T_cw, view_off, p_w, radius, bias, radius_px, status)) return VC_ERR_BAD_ARG;
  return vc::dot_bias_run(device, n_views, view_model, view_K, view_T_cw, view_off, p_w, radius, bias, radius_px, status, 0, nullptr);
}

extern "C" int vc_time_dot_bias_batch(int device, int n_views, const int* view_model, const double* view_K, const double* view_T_cw, const int* view_off,
                                      const double* p_w, const double* radius, int reps, double* kernel_ms) {
  if (reps < 1 || !kernel_ms || n_views < 1 || !view_off || view_off[0] < 0 || view_off[n_views] <= view_off[0]) return VC_ERR_BAD_ARG;
  const size_t end = (size_t)view_off[n_views];
  std::vector<double> bias(2 * end), radius_px(end);
  std::vector<int> status(end);
  if (!vc::dot_bias_args_ok(n_views, view_model, view_K, view_T_cw, view_off, p_w, radius, bias.data(), radius_px.data(), status.data())) return VC_ERR_BAD_ARG;
  return vc::dot_bias_run(device, n_views, view_model, view_K, view_T_cw, view_off, p_w, radius, bias.data(), radius_px.data(), status.data(), reps, kernel_ms);
}
