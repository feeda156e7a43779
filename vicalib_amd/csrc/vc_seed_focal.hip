// vc_seed_focal.hip -- the focal length of every camera from the homographies of its views of the planar target (gfx950, wave64, fp64
// throughout): vc_seed_focal_batch.  vc_seed_focal.hpp has the arithmetic, vc_seed.hpp the DLT and the eigen-solve it shares with the pose seed.
//
//  k_seed_focal_views   one wavefront per view, four views per workgroup, no block barrier, no LDS, no work array: the lanes stride over the
//                       view's corners, a corner's pixel relative to the principal point is formed where it is used.  Every sum over the
//                       corners is the fixed-order xor butterfly; every branch behind a sum is wave-uniform; the view index is scalar.
//  k_seed_focal_cams    one wavefront per camera: the lanes stride over THAT CAMERA'S views in view order (a list the host builds from
//                       view_cam), then the butterfly.  Which lane holds a view depends on its rank among its camera's views only, so the
//                       views of other cameras in the batch do not change a camera's bits.
// No floating-point atomic.  No CPU fallback: without a device the entry point fails.
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstring>
#include <vector>
#include "../../include/vicalib_amd.h"
#include "vc_kutil.hpp"
#include "vc_hostutil.hpp"
#include "vc_seed_focal.hpp"

namespace {

struct FocalBatch {
  int n_views, n_cams, min_corners;
  double max_fit, sin4;
  const int* view_cam;    // n_views
  const double* cam_pp;   // n_cams x 2
  const double* cam_R;    // n_cams
  const int* off;         // n_views + 1
  const double* pw;       // total x 3
  const double* uv;       // total x 2
  const int* cam_off;     // n_cams + 1: camera c owns cam_list[cam_off[c] .. cam_off[c + 1] - 1]
  const int* cam_list;    // n_views: the views of camera 0 in view order, then those of camera 1, ...
  double* H;              // n_views x 9
  double* rows;           // n_views x 4
  double* f;
  double* fit;
  int* used;
  int* status;
  double* cam_f;
  int* cam_views;
  int* cam_status;
};

struct FocalWave {
  static constexpr int kLanes = 64;
  int lane;
  __device__ __forceinline__ double allsum(double x) const { return vc::wave_allsum(x); }
  __device__ __forceinline__ int allsum(int x) const { return vc::wave_allsum(x); }
  __device__ __forceinline__ double bcast(double x, int j) const { return vc::readlane_f64(x, j); }
  __device__ __forceinline__ int bcast(int x, int j) const { return __builtin_amdgcn_readlane(x, j); }
  __device__ __forceinline__ int allmin(int x) const {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { const int y = __shfl_xor(x, o, 64); x = y < x ? y : x; }
    return x;
  }
};

__global__ __launch_bounds__(256) void k_seed_focal_views(FocalBatch b) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int v = __builtin_amdgcn_readfirstlane(blockIdx.x * 4 + wave);      // (scalar: the view's camera, principal point and pointers are loaded once per wave)
  if (v >= b.n_views) return;                                     // (a whole wave leaves: nothing in this kernel waits for another wave)
  const size_t o0 = (size_t)b.off[v];
  const int c = b.view_cam[v];
  vc::FocalView s;
  s.n = b.off[v + 1] - b.off[v];
  s.pw = b.pw + 3 * o0; s.uv = b.uv + 2 * o0;
  s.cx = b.cam_pp[2 * (size_t)c]; s.cy = b.cam_pp[2 * (size_t)c + 1]; s.R = b.cam_R[c];
  vc::FocalViewOut o;
  const int status = vc::focal_view(FocalWave{lane}, s, b.min_corners, b.max_fit, b.sin4, &o);
  if (lane == 0) {
    b.status[v] = status;
    if (status == vc::kFocalOk) {
#pragma unroll
      for (int k = 0; k < 9; ++k) b.H[(size_t)v * 9 + k] = o.H[k];
#pragma unroll
      for (int k = 0; k < 4; ++k) b.rows[(size_t)v * 4 + k] = o.rows[k];
      b.f[v] = o.f; b.fit[v] = o.fit_px; b.used[v] = o.used;
    }
  }
}

__global__ __launch_bounds__(256) void k_seed_focal_cams(FocalBatch b) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int c = __builtin_amdgcn_readfirstlane(blockIdx.x * 4 + wave);
  if (c >= b.n_cams) return;
  const int l0 = b.cam_off[c], n_list = b.cam_off[c + 1] - l0;
  double f = 0.0;
  int n_used = 0;
  const int status = vc::focal_cam(FocalWave{lane}, n_list, b.cam_list + l0, b.status, b.rows, b.sin4, &f, &n_used);
  if (lane == 0) {
    b.cam_status[c] = status; b.cam_views[c] = n_used;
    if (status == vc::kFocalCamOk) b.cam_f[c] = f;
  }
}

}  // namespace

namespace vc {

bool seed_focal_args_ok(int n_views, const int* view_cam, int n_cams, const double* cam_pp, const double* cam_radius, const int* view_off,
                        const double* p_w, const double* p_c, double max_fit_px, double min_tilt_deg, const double* view_rows, const double* view_f,
                        const double* view_fit_px, const int* view_used, const int* view_status, const double* cam_f, const int* cam_views,
                        const int* cam_status) {
  if (n_views < 0 || n_cams < 1 || !view_cam || !cam_pp || !cam_radius || !view_off || !p_w || !p_c || !view_rows || !view_f || !view_fit_px ||
      !view_used || !view_status || !cam_f || !cam_views || !cam_status)
    return false;
  if (!(max_fit_px >= 0.0) || !(min_tilt_deg > 0.0 && min_tilt_deg < 90.0) || view_off[0] < 0) return false;
  for (int c = 0; c < 2 * n_cams; ++c)
    if (!seed_finite(cam_pp[c])) return false;
  for (int v = 0; v < n_views; ++v)
    if (view_off[v + 1] < view_off[v] || view_cam[v] < 0 || view_cam[v] >= n_cams) return false;
  return true;
}

int seed_focal_run(int device, int n_views, const int* view_cam, int n_cams, const double* cam_pp, const double* cam_radius, const int* view_off,
                   const double* p_w, const double* p_c, int min_corners, double max_fit_px, double min_tilt_deg, double* view_H, double* view_rows,
                   double* view_f, double* view_fit_px, int* view_used, int* view_status, double* cam_f, int* cam_views, int* cam_status, int time_reps,
                   double* kernel_ms) {
  if (kernel_ms) *kernel_ms = 0.0;
  if (vch::open_device(device) != VC_OK) return VC_ERR_NO_DEVICE;
  hipStream_t stream = nullptr;
  const size_t total = n_views > 0 ? (size_t)view_off[n_views] : 0, nv = (size_t)n_views, nc = (size_t)n_cams;
  // the views of every camera in view order
  std::vector<int> cam_off(nc + 1, 0), cam_list(nv > 0 ? nv : 1);
  for (size_t v = 0; v < nv; ++v) ++cam_off[(size_t)view_cam[v] + 1];
  for (size_t c = 0; c < nc; ++c) cam_off[c + 1] += cam_off[c];
  {
    std::vector<int> at(cam_off.begin(), cam_off.end() - 1);
    for (size_t v = 0; v < nv; ++v) cam_list[(size_t)at[(size_t)view_cam[v]]++] = (int)v;
  }
  FocalBatch b;
  std::memset(&b, 0, sizeof(b));
  b.n_views = n_views; b.n_cams = n_cams; b.min_corners = min_corners; b.max_fit = max_fit_px; b.sin4 = focal_sin4(min_tilt_deg);
  int *d_view_cam = nullptr, *d_off = nullptr, *d_cam_off = nullptr, *d_cam_list = nullptr;
  double *d_pp = nullptr, *d_R = nullptr, *d_pw = nullptr, *d_uv = nullptr;
  auto carve = [&](vch::Carver q) {
    d_view_cam = q.take<int>(nv + 1); d_pp = q.take<double>(2 * nc); d_R = q.take<double>(nc); d_off = q.take<int>(nv + 1);
    d_pw = q.take<double>(3 * total + 1); d_uv = q.take<double>(2 * total + 1); d_cam_off = q.take<int>(nc + 1); d_cam_list = q.take<int>(nv + 1);
    b.H = q.take<double>(nv * 9 + 1); b.rows = q.take<double>(nv * 4 + 1); b.f = q.take<double>(nv + 1); b.fit = q.take<double>(nv + 1);
    b.used = q.take<int>(nv + 1); b.status = q.take<int>(nv + 1);
    b.cam_f = q.take<double>(nc); b.cam_views = q.take<int>(nc); b.cam_status = q.take<int>(nc);
    return q.bytes();
  };
  unsigned char* d_buf = nullptr;
  if (hipMalloc((void**)&d_buf, carve(vch::Carver())) != hipSuccess) return VC_ERR_NO_DEVICE;
  carve(vch::Carver(d_buf));
  b.view_cam = d_view_cam; b.cam_pp = d_pp; b.cam_R = d_R; b.off = d_off; b.pw = d_pw; b.uv = d_uv; b.cam_off = d_cam_off; b.cam_list = d_cam_list;
  std::vector<double> h_H(nv * 9), h_rows(nv * 4), h_f(nv), h_fit(nv), h_cam_f(nc);
  std::vector<int> h_used(nv), h_cam_status(nc);
  auto up = [&](void* dst, const void* src, size_t bytes) { return bytes == 0 || hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, stream) == hipSuccess; };
  auto down = [&](void* dst, const void* src, size_t bytes) { return bytes == 0 || hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, stream) == hipSuccess; };
  auto launch = [&]() {
    if (n_views > 0) hipLaunchKernelGGL(k_seed_focal_views, dim3((n_views + 3) / 4), dim3(256), 0, stream, b);
    hipLaunchKernelGGL(k_seed_focal_cams, dim3((n_cams + 3) / 4), dim3(256), 0, stream, b);
  };
  bool ok = up(d_view_cam, view_cam, nv * 4) && up(d_pp, cam_pp, nc * 16) && up(d_R, cam_radius, nc * 8) && up(d_off, view_off, nv > 0 ? (nv + 1) * 4 : 0) &&
            up(d_pw, p_w, total * 24) && up(d_uv, p_c, total * 16) && up(d_cam_off, cam_off.data(), (nc + 1) * 4) && up(d_cam_list, cam_list.data(), nv * 4);
  if (ok) {
    launch();
    ok = hipGetLastError() == hipSuccess && down(h_H.data(), b.H, nv * 72) && down(h_rows.data(), b.rows, nv * 32) && down(h_f.data(), b.f, nv * 8) &&
         down(h_fit.data(), b.fit, nv * 8) && down(h_used.data(), b.used, nv * 4) && down(view_status, b.status, nv * 4) &&
         down(h_cam_f.data(), b.cam_f, nc * 8) && down(cam_views, b.cam_views, nc * 4) && down(h_cam_status.data(), b.cam_status, nc * 4);
  }
  ok = hipStreamSynchronize(stream) == hipSuccess && ok;
  if (ok && kernel_ms && time_reps > 0)                              // (the kernels again on the same input: they write the same bits)
    ok = vch::time_back_to_back(stream, time_reps, launch, kernel_ms) == VC_OK;
  (void)hipFree(d_buf);
  if (!ok) return VC_ERR_NO_DEVICE;
  for (size_t v = 0; v < nv; ++v) {                                // a refused view's outputs are the caller's, untouched
    if (view_status[v] != kFocalOk) continue;
    if (view_H) std::memcpy(view_H + 9 * v, &h_H[9 * v], 72);
    std::memcpy(view_rows + 4 * v, &h_rows[4 * v], 32);
    view_f[v] = h_f[v]; view_fit_px[v] = h_fit[v]; view_used[v] = h_used[v];
  }
  for (size_t c = 0; c < nc; ++c) {
    cam_status[c] = h_cam_status[c];
    if (cam_status[c] == kFocalCamOk) cam_f[c] = h_cam_f[c];
  }
  return VC_OK;
}

}  // namespace vc

extern "C" int vc_seed_focal_batch(int device, int n_views, const int* view_cam, int n_cams, const double* cam_pp, const double* cam_radius,
                                   const int* view_off, const double* p_w, const double* p_c, int min_corners, double max_fit_px, double min_tilt_deg,
                                   double* view_H, double* view_rows, double* view_f, double* view_fit_px, int* view_used, int* view_status,
                                   double* cam_f, int* cam_views, int* cam_status) {
  if (!vc::seed_focal_args_ok(n_views, view_cam, n_cams, cam_pp, cam_radius, view_off, p_w, p_c, max_fit_px, min_tilt_deg, view_rows, view_f, view_fit_px,
                              view_used, view_status, cam_f, cam_views, cam_status))
    return VC_ERR_BAD_ARG;
  return vc::seed_focal_run(device, n_views, view_cam, n_cams, cam_pp, cam_radius, view_off, p_w, p_c, min_corners, max_fit_px, min_tilt_deg, view_H,
                            view_rows, view_f, view_fit_px, view_used, view_status, cam_f, cam_views, cam_status, 0, nullptr);
}

extern "C" int vc_time_seed_focal_batch(int device, int n_views, const int* view_cam, int n_cams, const double* cam_pp, const double* cam_radius,
                                        const int* view_off, const double* p_w, const double* p_c, int min_corners, double max_fit_px,
                                        double min_tilt_deg, int reps, double* kernel_ms) {
  if (reps < 1 || !kernel_ms || n_views < 1 || n_cams < 1) return VC_ERR_BAD_ARG;
  std::vector<double> rows(4 * (size_t)n_views), f(n_views), fit(n_views), cam_f(n_cams);
  std::vector<int> used(n_views), status(n_views), cam_views(n_cams), cam_status(n_cams);
  if (!vc::seed_focal_args_ok(n_views, view_cam, n_cams, cam_pp, cam_radius, view_off, p_w, p_c, max_fit_px, min_tilt_deg, rows.data(), f.data(), fit.data(),
                              used.data(), status.data(), cam_f.data(), cam_views.data(), cam_status.data()))
    return VC_ERR_BAD_ARG;
  return vc::seed_focal_run(device, n_views, view_cam, n_cams, cam_pp, cam_radius, view_off, p_w, p_c, min_corners, max_fit_px, min_tilt_deg, nullptr,
                            rows.data(), f.data(), fit.data(), used.data(), status.data(), cam_f.data(), cam_views.data(), cam_status.data(), reps, kernel_ms);
}
