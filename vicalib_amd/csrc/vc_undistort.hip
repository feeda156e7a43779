// vc_undistort.hip -- using the calibration: images and pixels of a calibrated camera mapped to an ideal pinhole camera on the GPU.
//
// What a caller of the reference does with cameras.xml through Calibu (Unproject, lookup-table rectification; tracker.cc:82-85 works
// with a loaded model and K().inverse()).  A vc_undistorter holds one source camera (any of the six models), one destination pinhole
// camera (fu fv u0 v0, size) and the rotation between them; it builds the lookup table once and then resamples batches of 8-bit images.
//
//   k_undist_map     one destination pixel per thread: ray = R_sd ((i - u0_d) / fu_d, (j - v0_d) / fv_d, 1) through the source model
//                    (project_any) -> the source coordinate as an fp32 pair; NaN pair = no source pixel
//   k_undist_remap   bilinear resampling of a batch of images through the map: four consecutive destination pixels per thread (two
//                    16-byte map loads, one 4-byte store), the image index in the grid; the byte gathers of neighbouring destination
//                    pixels hit neighbouring source bytes and are left to L2 (no LDS)
//   k_undist_points  one distorted source pixel per thread -> pixel of the destination camera: Newton on the radial profile with the
//                    analytic slope (vc_undistort.hpp), rotation, pinhole projection; branches per lane, no LDS, no atomics
// Pixel centres are at integers, as in the detector (vc_detect.hip).  No CPU fallback: vc_undistorter_create fails with
// VC_ERR_NO_DEVICE without a HIP device.  vc_undistort_fit_linear is host code and needs none.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>
#include "../../include/vicalib_amd.h"
#include "vc_hostutil.hpp"
#include "vc_undistort.hpp"

namespace {

using vc::UndistPlan;
constexpr int kMaxSize = 8192;
constexpr int kTimePoints = 65536;

__global__ __launch_bounds__(256) void k_undist_map(UndistPlan p, float2* __restrict__ map) {
  const int i = blockIdx.x * 256 + threadIdx.x, j = blockIdx.y;
  if (i >= p.map_pitch) return;                       // (j < dst_h by the grid)
  double x, y;
  const bool ok = i < p.dst_w && vc::undist_map_entry(p, i, j, &x, &y);
  const float nan = __builtin_nanf("");
  map[(size_t)j * p.map_pitch + i] = ok ? make_float2((float)x, (float)y) : make_float2(nan, nan);
}

// One destination pixel: (1 - ay) ((1 - ax) p00 + ax p01) + ay ((1 - ax) p10 + ax p11) in fp64, rounded half-up.  x0 = min(floor(x), w - 2):
// x = w - 1 reads columns w - 2 and w - 1 with weight 1 on the last one and never column w (the map holds no coordinate outside
// [0, w - 1] x [0, h - 1]).  A thread owns four consecutive destination pixels of one image (the image's index is the grid's y).  Nothing is
// conditional on an entry's validity: a NaN coordinate becomes 0 through fmaxf, an invalid entry reads the image's first pixels and its value
// is blended away against the fill value with weights 0 and 1, so that the compiler keeps the two 16-byte map loads whole and has the gathers
// of a thread's four pixels in flight together.  (Owning the four pixels of 8 images per thread, to read the
// 8-byte map entries once per group, was measured and is not faster: DESIGN 4.7.)
__global__ __launch_bounds__(256) void k_undist_remap(UndistPlan p, const float2* __restrict__ map, const unsigned char* __restrict__ src, int src_pitch,
                                                      size_t src_stride, unsigned char* __restrict__ dst, int dst_pitch, size_t dst_stride) {
  const int qpr = p.map_pitch >> 2;                          // quads of destination pixels per row
  const int t = blockIdx.x * 256 + threadIdx.x;
  if (t >= qpr * p.dst_h) return;
  const int j = t / qpr, i = (t - j * qpr) << 2;
  const float4* m = reinterpret_cast<const float4*>(map + (size_t)j * p.map_pitch + i);      // 32-byte aligned: map_pitch is a multiple of 4
  const float4 m0 = m[0], m1 = m[1];
  const float fx[4] = {m0.x, m0.z, m1.x, m1.z}, fy[4] = {m0.y, m0.w, m1.y, m1.w};
  const unsigned char* s = src + (size_t)blockIdx.y * src_stride;
  double ax[4], ay[4];
  unsigned p00[4], p01[4], p10[4], p11[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const double x = (double)fmaxf(fx[k], 0.0f), y = (double)fmaxf(fy[k], 0.0f);      // valid coordinates are >= 0; a NaN becomes 0 (maxNum)
    const int x0 = min((int)floor(x), p.src_w - 2), y0 = min((int)floor(y), p.src_h - 2);
    ax[k] = x - (double)x0; ay[k] = y - (double)y0;
    const unsigned char* r0 = s + (size_t)y0 * src_pitch + x0;
    p00[k] = r0[0]; p01[k] = r0[1]; p10[k] = r0[src_pitch]; p11[k] = r0[src_pitch + 1];
  }
  unsigned v[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const double val = (1.0 - ay[k]) * ((1.0 - ax[k]) * (double)p00[k] + ax[k] * (double)p01[k]) + ay[k] * ((1.0 - ax[k]) * (double)p10[k] + ax[k] * (double)p11[k]);
    const double okf = fx[k] == fx[k] ? 1.0 : 0.0;             // val * 1 + fill * 0 and val * 0 + fill * 1 are exact: arithmetic, not a branch
    v[k] = (unsigned)min(max((int)floor(okf * val + (1.0 - okf) * (double)p.fill + 0.5), 0), 255);
  }
  unsigned char* d = dst + (size_t)blockIdx.y * dst_stride + (size_t)j * dst_pitch + i;
  if (i + 3 < p.dst_w && (reinterpret_cast<size_t>(d) & 3) == 0) {
    *reinterpret_cast<unsigned*>(d) = v[0] | (v[1] << 8) | (v[2] << 16) | (v[3] << 24);
  } else {                                                   // a row's tail, or rows that do not start on a 4-byte boundary
    if (i < p.dst_w) d[0] = (unsigned char)v[0];
    if (i + 1 < p.dst_w) d[1] = (unsigned char)v[1];
    if (i + 2 < p.dst_w) d[2] = (unsigned char)v[2];
    if (i + 3 < p.dst_w) d[3] = (unsigned char)v[3];
  }
}

__global__ __launch_bounds__(256) void k_undist_points(UndistPlan p, int n, const double2* __restrict__ in, double2* __restrict__ out,
                                                       unsigned char* __restrict__ valid) {
  const int k = blockIdx.x * 256 + threadIdx.x;
  if (k >= n) return;
  const double2 q = in[k];
  double a, b;
  const bool ok = vc::undist_point(p, q.x, q.y, &a, &b);
  const double nan = __builtin_nan("");
  out[k] = ok ? make_double2(a, b) : make_double2(nan, nan);
  valid[k] = ok ? 1 : 0;
}

bool model_args_ok(int model, const double* params, int nparams, int w, int h) {
  if (model < 0 || model > 5 || !params || nparams != vc::model_nk(model)) return false;
  if (w < 2 || h < 2 || w > kMaxSize || h > kMaxSize) return false;
  for (int k = 0; k < nparams; ++k) if (!std::isfinite(params[k])) return false;
  return params[0] != 0.0 && params[1] != 0.0;
}
bool linear_ok(const double* dl) { return dl && std::isfinite(dl[0]) && std::isfinite(dl[1]) && std::isfinite(dl[2]) && std::isfinite(dl[3]) && dl[0] != 0.0 && dl[1] != 0.0; }

}  // namespace

struct vc_undistorter {
  int device = 0;
  UndistPlan p;
  hipStream_t stream = nullptr;
  float2* d_map = nullptr;
  // staging of the host entry points (rows packed; destination rows at map_pitch bytes), grown to the largest batch seen
  unsigned char* d_src = nullptr; unsigned char* d_dst = nullptr; unsigned char* h_src = nullptr; unsigned char* h_dst = nullptr;
  int cap_images = 0;
  double* d_pts = nullptr; double* h_pts = nullptr;      // [in: 2 n doubles | out: 2 n doubles | valid: n bytes]
  int cap_points = 0;
  bool in_flight = false;        // a call left through an error path: the stream may still read the staging buffers
  size_t src_bytes() const { return (size_t)p.src_w * p.src_h; }
  size_t dst_bytes() const { return (size_t)p.map_pitch * p.dst_h; }
};

namespace {

void launch_map(vc_undistorter* u) {
  hipLaunchKernelGGL(k_undist_map, dim3((u->p.map_pitch + 255) / 256, u->p.dst_h), dim3(256), 0, u->stream, u->p, u->d_map);
}
void launch_remap(vc_undistorter* u, int n, const unsigned char* src, int src_pitch, size_t src_stride, unsigned char* dst, int dst_pitch, size_t dst_stride) {
  const int threads = (u->p.map_pitch >> 2) * u->p.dst_h;
  hipLaunchKernelGGL(k_undist_remap, dim3((threads + 255) / 256, n), dim3(256), 0, u->stream, u->p, u->d_map, src, src_pitch, src_stride, dst, dst_pitch, dst_stride);
}
void launch_points(vc_undistorter* u, int n) {
  double* in = u->d_pts; double* out = in + 2 * (size_t)u->cap_points;
  unsigned char* valid = reinterpret_cast<unsigned char*>(out + 2 * (size_t)u->cap_points);
  hipLaunchKernelGGL(k_undist_points, dim3((n + 255) / 256), dim3(256), 0, u->stream, u->p, n, reinterpret_cast<const double2*>(in), reinterpret_cast<double2*>(out), valid);
}
bool reserve_images(vc_undistorter* u, int n) {
  if (n <= u->cap_images) return true;
  (void)hipStreamSynchronize(u->stream);
  (void)hipFree(u->d_src); (void)hipFree(u->d_dst);
  if (u->h_src) (void)hipHostFree(u->h_src);
  if (u->h_dst) (void)hipHostFree(u->h_dst);
  u->d_src = u->d_dst = u->h_src = u->h_dst = nullptr; u->cap_images = 0;
  const size_t sb = u->src_bytes() * n, db = u->dst_bytes() * n;
  if (hipMalloc((void**)&u->d_src, sb) != hipSuccess || hipMalloc((void**)&u->d_dst, db) != hipSuccess ||
      hipHostMalloc((void**)&u->h_src, sb, hipHostMallocDefault) != hipSuccess || hipHostMalloc((void**)&u->h_dst, db, hipHostMallocDefault) != hipSuccess) return false;
  u->cap_images = n;
  return true;
}
size_t points_bytes(int n) { return (size_t)n * 33; }
// a batch of n images at src / dst (host or device), rows and images at the given pitches and strides
bool images_args_ok(const vc_undistorter* u, int n, const unsigned char* src, int src_pitch, long long src_stride, const unsigned char* dst, int dst_pitch,
                    long long dst_stride) {
  if (!u || n < 0 || (n > 0 && (!src || !dst)) || src_pitch < u->p.src_w || dst_pitch < u->p.dst_w) return false;
  if (n > 1 && (src_stride < (long long)src_pitch * u->p.src_h || dst_stride < (long long)dst_pitch * u->p.dst_h)) return false;
  return n <= 65535;                                         // (the image index is the grid's y)
}
bool reserve_points(vc_undistorter* u, int n) {
  if (n <= u->cap_points) return true;
  (void)hipStreamSynchronize(u->stream);
  (void)hipFree(u->d_pts);
  if (u->h_pts) (void)hipHostFree(u->h_pts);
  u->d_pts = u->h_pts = nullptr; u->cap_points = 0;
  n = (n + 63) & ~63;
  if (hipMalloc((void**)&u->d_pts, points_bytes(n)) != hipSuccess || hipHostMalloc((void**)&u->h_pts, points_bytes(n), hipHostMallocDefault) != hipSuccess) return false;
  u->cap_points = n;
  return true;
}

}  // namespace

extern "C" {

int vc_undistorter_create(int device, int model, const double* params, int nparams, int src_w, int src_h, const double dst_linear[4], int dst_w, int dst_h,
                          const double R_ds[9], int fill, vc_undistorter** out) {
  if (!out || !model_args_ok(model, params, nparams, src_w, src_h) || !dst_linear || !vc::undist_dest_args_ok(dst_linear, dst_w, dst_h, fill)) return VC_ERR_BAD_ARG;
  if (R_ds && !vc::is_rotation(R_ds)) return VC_ERR_BAD_ARG;
  if (vch::open_device(device) != VC_OK) return VC_ERR_NO_DEVICE;
  vc_undistorter* u = new vc_undistorter;
  u->device = device;
  UndistPlan& p = u->p;
  vc::undist_source_plan(&p, model, params, nparams, src_w, src_h, R_ds);
  p.dst_w = dst_w; p.dst_h = dst_h; p.map_pitch = (dst_w + 3) & ~3; p.fill = fill;
  for (int k = 0; k < 4; ++k) p.dl[k] = dst_linear[k];
  if (hipStreamCreate(&u->stream) != hipSuccess || hipMalloc((void**)&u->d_map, (size_t)p.map_pitch * dst_h * sizeof(float2)) != hipSuccess) { vc_undistorter_destroy(u); return VC_ERR_NO_DEVICE; }
  launch_map(u);                                     // the map is built once
  if (hipGetLastError() != hipSuccess || hipStreamSynchronize(u->stream) != hipSuccess) { vc_undistorter_destroy(u); return VC_ERR_NO_DEVICE; }
  *out = u;
  return VC_OK;
}
void vc_undistorter_destroy(vc_undistorter* u) {
  if (!u) return;
  (void)hipSetDevice(u->device);
  if (u->stream) { (void)hipStreamSynchronize(u->stream); (void)hipStreamDestroy(u->stream); }
  (void)hipFree(u->d_map); (void)hipFree(u->d_src); (void)hipFree(u->d_dst); (void)hipFree(u->d_pts);
  if (u->h_src) (void)hipHostFree(u->h_src);
  if (u->h_dst) (void)hipHostFree(u->h_dst);
  if (u->h_pts) (void)hipHostFree(u->h_pts);
  delete u;
}

}  // extern "C"

// The fit behind vc_undistort_fit_linear (one side, identity rotation) and vc_stereo_fit_linear (two sides, their rectifying rotations):
// one destination camera for all sides.  side[k] holds the source model, its size and R_sd; dst_w / dst_h / dl are filled in here.  With one
// side and the identity rotation every product with R is exact, so the single-camera fit returns what it did before it was shared.
int vc::undist_fit_sides(int n_sides, UndistPlan* side, int dst_w, int dst_h, double alpha, double dst_linear[4]) {
  // the source borders in the pinhole plane: the corners and 64 points inside every edge.  Edge e: 0 left, 1 right, 2 top, 3 bottom; a corner
  // belongs to both of its edges.
  double lo[4] = {-HUGE_VAL, HUGE_VAL, -HUGE_VAL, HUGE_VAL};      // innermost coordinate seen on every edge: max of the left edges' x, min of the right, ...
  double box[4] = {HUGE_VAL, -HUGE_VAL, HUGE_VAL, -HUGE_VAL};     // bounding box x0 x1 y0 y1 (of all sides: their union)
  for (int k = 0; k < n_sides; ++k) {
    UndistPlan& p = side[k];
    p.dst_w = dst_w; p.dst_h = dst_h;
    const double xm = p.src_w - 1.0, ym = p.src_h - 1.0;
    const double* R = p.R_sd;
    int kept = 0;
    auto sample = [&](double u, double v, int e0, int e1) {
      double s[3];
      if (!vc::undist_unproject(p.model, p.K, p.pre, u, v, s)) return;
      const double r[3] = {R[0] * s[0] + R[3] * s[1] + R[6] * s[2], R[1] * s[0] + R[4] * s[1] + R[7] * s[2], R[2] * s[0] + R[5] * s[1] + R[8] * s[2]};      // R_ds s
      if (!(r[2] > 0.0)) return;        // no pinhole image
      const double x = r[0] / r[2], y = r[1] / r[2];
      if (!std::isfinite(x) || !std::isfinite(y)) return;
      ++kept;
      box[0] = std::min(box[0], x); box[1] = std::max(box[1], x); box[2] = std::min(box[2], y); box[3] = std::max(box[3], y);
      for (int e : {e0, e1}) {
        if (e == 0) lo[0] = std::max(lo[0], x);
        if (e == 1) lo[1] = std::min(lo[1], x);
        if (e == 2) lo[2] = std::max(lo[2], y);
        if (e == 3) lo[3] = std::min(lo[3], y);
      }
    };
    sample(0, 0, 0, 2); sample(xm, 0, 1, 2); sample(0, ym, 0, 3); sample(xm, ym, 1, 3);
    for (int i = 1; i <= 64; ++i) {
      const double s = i / 65.0;
      sample(0, s * ym, 0, -1); sample(xm, s * ym, 1, -1); sample(s * xm, 0, 2, -1); sample(s * xm, ym, 3, -1);
    }
    if (kept < 8) return VC_ERR_NUMERIC;
  }
  if (!(lo[0] < lo[1]) || !(lo[2] < lo[3]) || !(box[0] < box[1]) || !(box[2] < box[3])) return VC_ERR_NUMERIC;      // (two sides: an empty intersection)
  // alpha = 0: the rectangle between the edges' innermost samples.  The samples miss an edge's true innermost point by a little, so the
  // rectangle is then drawn in until every pixel of the destination image's border has a source pixel on every side (same test as the map
  // kernel's).
  double dl[4];
  auto to_linear = [&](const double* r, double* d) {
    d[0] = (dst_w - 1.0) / (r[1] - r[0]); d[2] = -r[0] * d[0];
    d[1] = (dst_h - 1.0) / (r[3] - r[2]); d[3] = -r[2] * d[1];
  };
  // Only the destination image's border is probed: the destination pixels that have a source pixel are the preimage of the source rectangle
  // under a map that is continuous and one-to-one on the field the border samples span, a region without holes, so a closed border inside it
  // has its interior inside it too.
  double in[4] = {lo[0], lo[1], lo[2], lo[3]}, gain[4] = {1.5, 1.5, 1.5, 1.5};
  bool inside = false;
  for (int round = 0; round < 64 && !inside; ++round) {
    to_linear(in, dl);
    // by how far the worst pixel of each side of the destination border misses a source image, as the step it asks for in the pinhole plane:
    // the miss in source pixels over that source's focal length, times a gain that doubles while the side keeps missing (far off the axis of a
    // fisheye a step in the pinhole plane moves the source pixel by a small fraction of what it does at the centre)
    double step[4] = {0, 0, 0, 0};
    for (int k = 0; k < n_sides; ++k) {
      const UndistPlan& p = side[k];
      const double xm = p.src_w - 1.0, ym = p.src_h - 1.0;
      const double* R = p.R_sd;
      double miss[4] = {0, 0, 0, 0};
      auto probe = [&](int i, int j, int e) {
        const double a = ((double)i - dl[2]) / dl[0], b = ((double)j - dl[3]) / dl[1];
        const double ray[3] = {R[0] * a + R[1] * b + R[2], R[3] * a + R[4] * b + R[5], R[6] * a + R[7] * b + R[8]};
        double pix[2];
        vc::project_any<false>(p.model, ray, p.K, p.pre, pix, nullptr, nullptr);
        double d = std::max(std::max(-pix[0], pix[0] - xm), std::max(-pix[1], pix[1] - ym));
        if (!std::isfinite(d) || (!(ray[2] > 0.0) && p.model != vc::kKb4)) d = 1.0;
        if (d > vc::kUndistBorderTol) miss[e] = std::max(miss[e], d);
      };
      for (int j = 0; j < dst_h; ++j) { probe(0, j, 0); probe(dst_w - 1, j, 1); }
      for (int i = 0; i < dst_w; ++i) { probe(i, 0, 2); probe(i, dst_h - 1, 3); }
      const double f[4] = {std::fabs(p.K[0]), std::fabs(p.K[0]), std::fabs(p.K[1]), std::fabs(p.K[1])};
      for (int e = 0; e < 4; ++e)
        if (miss[e] != 0.0) step[e] = std::max(step[e], gain[e] * miss[e] / f[e]);
    }
    if (step[0] == 0.0 && step[1] == 0.0 && step[2] == 0.0 && step[3] == 0.0) { inside = true; break; }
    for (int e = 0; e < 4; ++e) {
      if (step[e] == 0.0) continue;
      in[e] += ((e & 1) ? -1.0 : 1.0) * step[e];
      gain[e] *= 2.0;
    }
    if (!(in[0] < in[1]) || !(in[2] < in[3])) return VC_ERR_NUMERIC;
  }
  if (!inside) return VC_ERR_NUMERIC;               // never intrinsics that break alpha = 0's promise
  double r[4];
  for (int k = 0; k < 4; ++k) r[k] = (1.0 - alpha) * in[k] + alpha * box[k];
  to_linear(r, dst_linear);
  return VC_OK;
}
void vc::undist_source_plan(UndistPlan* p, int model, const double* params, int nparams, int src_w, int src_h, const double* R_ds) {
  std::memset(p, 0, sizeof(*p));
  p->model = model; p->src_w = src_w; p->src_h = src_h;
  for (int k = 0; k < nparams; ++k) p->K[k] = params[k];
  vc::model_precompute(model, p->K, &p->pre);
  for (int i = 0; i < 3; ++i) for (int j = 0; j < 3; ++j) p->R_sd[3 * i + j] = R_ds ? R_ds[3 * j + i] : (i == j ? 1.0 : 0.0);
}
bool vc::undist_source_args_ok(int model, const double* params, int nparams, int w, int h) { return model_args_ok(model, params, nparams, w, h); }
bool vc::undist_dest_args_ok(const double* dst_linear /* nullable */, int dst_w, int dst_h, int fill) {
  return (!dst_linear || linear_ok(dst_linear)) && dst_w >= 2 && dst_h >= 2 && dst_w <= kMaxSize && dst_h <= kMaxSize && fill >= 0 && fill <= 255;
}
const vc::UndistPlan& vc::undist_plan_of(const vc_undistorter* u) { return u->p; }

extern "C" {

int vc_undistort_fit_linear(int model, const double* params, int nparams, int src_w, int src_h, int dst_w, int dst_h, double alpha, double dst_linear[4]) {
  if (!model_args_ok(model, params, nparams, src_w, src_h) || !dst_linear || !vc::undist_dest_args_ok(nullptr, dst_w, dst_h, 0)) return VC_ERR_BAD_ARG;
  if (!(alpha >= 0.0 && alpha <= 1.0)) return VC_ERR_BAD_ARG;
  UndistPlan p;
  vc::undist_source_plan(&p, model, params, nparams, src_w, src_h, nullptr);
  return vc::undist_fit_sides(1, &p, dst_w, dst_h, alpha, dst_linear);
}

int vc_undistort_images_device(vc_undistorter* u, int n, const unsigned char* d_src, int src_pitch, long long src_stride, unsigned char* d_dst, int dst_pitch,
                               long long dst_stride) {
  if (!images_args_ok(u, n, d_src, src_pitch, src_stride, d_dst, dst_pitch, dst_stride)) return VC_ERR_BAD_ARG;
  if (n == 0) return VC_OK;
  if (hipSetDevice(u->device) != hipSuccess) return VC_ERR_NO_DEVICE;
  launch_remap(u, n, d_src, src_pitch, (size_t)src_stride, d_dst, dst_pitch, (size_t)dst_stride);
  return hipGetLastError() == hipSuccess ? VC_OK : VC_ERR_NO_DEVICE;
}
}  // extern "C"

// vc_undistort_images in two halves, so that a rectifier (vc_rectify.hip) has both sides' batches in flight before it waits for either:
// begin stages and enqueues upload, remap and download on the handle's stream; end waits for the stream and hands the pixels out.
int vc::undist_images_begin(vc_undistorter* u, int n, const unsigned char* src, int src_pitch, long long src_stride, unsigned char* dst, int dst_pitch, long long dst_stride) {
  if (!images_args_ok(u, n, src, src_pitch, src_stride, dst, dst_pitch, dst_stride)) return VC_ERR_BAD_ARG;
  if (n == 0) return VC_OK;
  if (hipSetDevice(u->device) != hipSuccess) return VC_ERR_NO_DEVICE;
  // one call in flight per handle (the staging buffers and the stream belong to it), as for a detector
  if (u->in_flight) (void)hipStreamSynchronize(u->stream);
  if (!reserve_images(u, n)) return VC_ERR_NO_DEVICE;
  u->in_flight = true;
  const int sw = u->p.src_w, sh = u->p.src_h, dp = u->p.map_pitch;
  for (int k = 0; k < n; ++k)
    for (int y = 0; y < sh; ++y) std::memcpy(u->h_src + ((size_t)k * sh + y) * sw, src + (size_t)k * src_stride + (size_t)y * src_pitch, (size_t)sw);
  if (hipMemcpyAsync(u->d_src, u->h_src, u->src_bytes() * n, hipMemcpyHostToDevice, u->stream) != hipSuccess) return VC_ERR_NO_DEVICE;
  launch_remap(u, n, u->d_src, sw, u->src_bytes(), u->d_dst, dp, u->dst_bytes());
  if (hipGetLastError() != hipSuccess || hipMemcpyAsync(u->h_dst, u->d_dst, u->dst_bytes() * n, hipMemcpyDeviceToHost, u->stream) != hipSuccess) return VC_ERR_NO_DEVICE;
  return VC_OK;
}
int vc::undist_images_end(vc_undistorter* u, int n, unsigned char* dst, int dst_pitch, long long dst_stride) {
  if (n == 0) return VC_OK;
  if (hipSetDevice(u->device) != hipSuccess || hipStreamSynchronize(u->stream) != hipSuccess) return VC_ERR_NO_DEVICE;
  u->in_flight = false;
  const int dw = u->p.dst_w, dh = u->p.dst_h, dp = u->p.map_pitch;
  for (int k = 0; k < n; ++k)                          // only the pixels: a destination row's padding is the caller's
    for (int y = 0; y < dh; ++y) std::memcpy(dst + (size_t)k * dst_stride + (size_t)y * dst_pitch, u->h_dst + ((size_t)k * dh + y) * dp, (size_t)dw);
  return VC_OK;
}
extern "C" {

int vc_undistort_images(vc_undistorter* u, int n, const unsigned char* src, int src_pitch, long long src_stride, unsigned char* dst, int dst_pitch, long long dst_stride) {
  const int rc = vc::undist_images_begin(u, n, src, src_pitch, src_stride, dst, dst_pitch, dst_stride);
  return rc != VC_OK ? rc : vc::undist_images_end(u, n, dst, dst_pitch, dst_stride);
}
void* vc_undistort_stream(vc_undistorter* u) { return u ? (void*)u->stream : nullptr; }

int vc_undistort_points(vc_undistorter* u, int n, const double* src_px, double* dst_px, unsigned char* valid) {
  if (!u || n < 0 || (n > 0 && (!src_px || !dst_px))) return VC_ERR_BAD_ARG;
  if (n == 0) return VC_OK;
  if (hipSetDevice(u->device) != hipSuccess) return VC_ERR_NO_DEVICE;
  if (u->in_flight) (void)hipStreamSynchronize(u->stream);
  if (!reserve_points(u, n)) return VC_ERR_NO_DEVICE;
  u->in_flight = true;
  const size_t cap = (size_t)u->cap_points;
  std::memcpy(u->h_pts, src_px, (size_t)n * 16);
  if (hipMemcpyAsync(u->d_pts, u->h_pts, (size_t)n * 16, hipMemcpyHostToDevice, u->stream) != hipSuccess) return VC_ERR_NO_DEVICE;
  launch_points(u, n);
  // results: out (2 n doubles at 2 cap) and valid (n bytes at 4 cap doubles) -- two copies, one synchronisation
  if (hipGetLastError() != hipSuccess ||
      hipMemcpyAsync(u->h_pts + 2 * cap, u->d_pts + 2 * cap, (size_t)n * 16, hipMemcpyDeviceToHost, u->stream) != hipSuccess ||
      hipMemcpyAsync(u->h_pts + 4 * cap, u->d_pts + 4 * cap, (size_t)n, hipMemcpyDeviceToHost, u->stream) != hipSuccess ||
      hipStreamSynchronize(u->stream) != hipSuccess) return VC_ERR_NO_DEVICE;
  u->in_flight = false;
  std::memcpy(dst_px, u->h_pts + 2 * cap, (size_t)n * 16);
  if (valid) std::memcpy(valid, u->h_pts + 4 * cap, (size_t)n);
  return VC_OK;
}

int vc_undistort_get_map(vc_undistorter* u, float* map, unsigned char* valid) {
  if (!u) return VC_ERR_BAD_ARG;
  if (!map && !valid) return VC_OK;
  if (hipSetDevice(u->device) != hipSuccess) return VC_ERR_NO_DEVICE;
  const int w = u->p.dst_w, h = u->p.dst_h, mp = u->p.map_pitch;
  std::vector<float> tmp((size_t)mp * h * 2);
  if (hipStreamSynchronize(u->stream) != hipSuccess || hipMemcpy(tmp.data(), u->d_map, tmp.size() * 4, hipMemcpyDeviceToHost) != hipSuccess) return VC_ERR_NO_DEVICE;
  for (int j = 0; j < h; ++j) {
    const float* row = tmp.data() + (size_t)j * mp * 2;
    if (map) std::memcpy(map + (size_t)j * w * 2, row, (size_t)w * 8);
    if (valid) for (int i = 0; i < w; ++i) valid[(size_t)j * w + i] = row[2 * i] == row[2 * i] ? 1 : 0;
  }
  return VC_OK;
}
int vc_undistort_get_linear(vc_undistorter* u, double dst_linear[4], int dst_size[2]) {
  if (!u) return VC_ERR_BAD_ARG;
  if (dst_linear) std::memcpy(dst_linear, u->p.dl, 32);
  if (dst_size) { dst_size[0] = u->p.dst_w; dst_size[1] = u->p.dst_h; }
  return VC_OK;
}

int vc_time_undistort(vc_undistorter* u, int n_images, int reps, double out_ms[3]) {
  if (!u || n_images < 1 || n_images > 65535 || reps < 1 || !out_ms) return VC_ERR_BAD_ARG;
  if (hipSetDevice(u->device) != hipSuccess) return VC_ERR_NO_DEVICE;
  if (u->in_flight) (void)hipStreamSynchronize(u->stream);
  if (!reserve_images(u, n_images) || !reserve_points(u, kTimePoints)) return VC_ERR_NO_DEVICE;
  // device-resident inputs: a grey ramp for the images, a lattice over the source image for the points
  for (size_t k = 0; k < u->src_bytes() * n_images; ++k) u->h_src[k] = (unsigned char)((k * 7) & 255);
  const int side = 256;
  for (int k = 0; k < kTimePoints; ++k) {
    u->h_pts[2 * k] = (u->p.src_w - 1.0) * (k % side) / (side - 1.0);
    u->h_pts[2 * k + 1] = (u->p.src_h - 1.0) * (k / side) / (side - 1.0);
  }
  if (hipMemcpyAsync(u->d_src, u->h_src, u->src_bytes() * n_images, hipMemcpyHostToDevice, u->stream) != hipSuccess ||
      hipMemcpyAsync(u->d_pts, u->h_pts, (size_t)kTimePoints * 16, hipMemcpyHostToDevice, u->stream) != hipSuccess) return VC_ERR_NO_DEVICE;
  for (int what = 0; what < 3; ++what) {
    auto launch = [&]() {                              // (the map a launch rewrites is the same map)
      if (what == 0) launch_map(u);
      else if (what == 1) launch_remap(u, n_images, u->d_src, u->p.src_w, u->src_bytes(), u->d_dst, u->p.map_pitch, u->dst_bytes());
      else launch_points(u, kTimePoints);
    };
    const int rc = vch::time_back_to_back(u->stream, reps, launch, &out_ms[what]);
    if (rc != VC_OK) return rc;
  }
  return VC_OK;
}

}  // extern "C"
