// vc_register.hip -- using the calibration of a depth camera and another camera of the rig: a depth image of the source camera S taken into
// the pixels of the destination camera D, and D's 8-bit image taken into S's pixels, on the GPU.  Definitions: include/vicalib_amd.h; the
// arithmetic: vc_register.hpp.
//
//   k_reg_rays       (vc_reg_rays.hpp) built once at create: the ray of every pixel centre (w_s x h_s) and of every node of the corner lattice
//                    ((w_s + 1) x (h_s + 1), node (i, j) at (i - 0.5, j - 0.5)) by Newton inversion; a ray is an fp64 pair (x, y) plus z, and
//                    z = NaN says that the position has no ray
//   k_reg_scatter    one thread per source pixel of the batch: a forward warp.  The depth test is ONE 64-bit atomicMin per destination pixel
//                    a candidate lands on, key = (w << 32) | source index, no returned value used: the minimum does not depend on the order
//                    of arrival, so the result is the same bits in every run.  The key buffer is cleared to all-ones on the stream first.
//                    Drop rules are counted per wavefront (ballot + popcount), one integer atomicAdd per wavefront and rule.
//   k_reg_resolve    keys -> the uint16 image and the int32 index map; four consecutive pixels per thread (two 16-byte key loads)
//   k_reg_gather     one thread per source pixel: visible where the depth test's winner at its projection is no nearer than occl_tol ->
//                    bilinear sample of D's image (double precision, rounded half-up), `fill` elsewhere
//   k_reg_points     the continuous face: (u, v, value) -> (q_x, q_y, m_d / unit_dst), Newton in the kernel
// No LDS, no float atomics.  No CPU fallback: vc_registrar_create fails with VC_ERR_NO_DEVICE without a HIP device.
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstring>
#include "../../include/vicalib_amd.h"
#include "vc_hostutil.hpp"
#include "vc_reg_rays.hpp"
#include "vc_register.hpp"

namespace {

using vc::RegisterPlan;
using vc::RegTables;
using vc::load_ray;
typedef unsigned long long u64;
constexpr int kTimePoints = 65536;
constexpr int kMaxImages = 65535;                      // (the image index is the grid's y)

// a batch of images of one camera: rows `pitch` bytes apart, images `stride` bytes apart
struct RegImages {
  unsigned char* p; int pitch; size_t stride;
};

// the lanes of this wavefront that hold `pred`, added to *counter by one atomic of lane 0
__device__ __forceinline__ void count_wave(bool pred, u64* counter) {
  const u64 b = __ballot(pred);
  if ((threadIdx.x & 63) == 0 && b) atomicAdd(counter, (u64)__popcll(b));
}

// keys: n x key_stride (key_stride >= w_d h_d); counters: n x 8
__global__ __launch_bounds__(256) void k_reg_scatter(RegisterPlan p, RegTables t, RegImages src, u64* __restrict__ keys, size_t key_stride, u64* __restrict__ counters) {
  const int ns = p.s.w * p.s.h;
  const int e = blockIdx.x * 256 + threadIdx.x, img = blockIdx.y;
  int code = -1;                                               // (a thread beyond the image counts nowhere)
  if (e < ns) {
    const int j = e / p.s.w, i = e - j * p.s.w;
    const unsigned value = *reinterpret_cast<const unsigned short*>(src.p + (size_t)img * src.stride + (size_t)j * src.pitch + 2 * (size_t)i);
    code = vc::kRegDropZero;
    if (value != 0) {
      double rc[3], ra[3] = {0, 0, 0}, rb[3] = {0, 0, 0};
      const bool okc = load_ray(t.c_xy, t.c_z, (size_t)e, rc);
      bool oka = true, okb = true;
      if (p.splat == vc::kRegFootprint) {
        const size_t a = (size_t)j * (p.s.w + 1) + i;
        oka = load_ray(t.l_xy, t.l_z, a, ra);
        okb = load_ray(t.l_xy, t.l_z, a + p.s.w + 2, rb);      // node (i + 1, j + 1)
      }
      unsigned w;
      vc::RegRect r;
      code = vc::reg_candidate(p, value, rc, okc, ra, oka, rb, okb, &w, &r);
      if (code == vc::kRegCandidates) {
        const u64 key = vc::reg_key(w, (unsigned)e);
        u64* k0 = keys + (size_t)img * key_stride;
        for (int y = r.y0; y <= r.y1; ++y)                     // (the rectangle is clipped to D's image: every index is below w_d h_d)
          for (int x = r.x0; x <= r.x1; ++x) atomicMin(k0 + (size_t)y * p.d.w + x, key);
      }
    }
  }
  u64* c = counters + (size_t)img * vc::kRegCounters;
#pragma unroll
  for (int rule = 0; rule <= vc::kRegCandidates; ++rule) count_wave(code == rule, c + rule);
}

// index (nullable): n x npix int32, packed
__global__ __launch_bounds__(256) void k_reg_resolve(int w_d, int npix, const u64* __restrict__ keys, size_t key_stride, RegImages dst, int* __restrict__ index,
                                                     u64* __restrict__ counters) {
  const int f = (blockIdx.x * 256 + threadIdx.x) << 2, img = blockIdx.y;
  u64 key[4] = {vc::kRegEmptyKey, vc::kRegEmptyKey, vc::kRegEmptyKey, vc::kRegEmptyKey};
  if (f < npix) {                                              // key_stride is a multiple of 4: the quad is inside the image's keys and 32-byte aligned
    const ulonglong2* k = reinterpret_cast<const ulonglong2*>(keys + (size_t)img * key_stride + f);
    const ulonglong2 a = k[0], b = k[1];
    key[0] = a.x; key[1] = a.y; key[2] = b.x; key[3] = b.y;
    int j = f / w_d, i = f - j * w_d;
    unsigned char* d = dst.p + (size_t)img * dst.stride;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      if (f + q >= npix) { key[q] = vc::kRegEmptyKey; continue; }      // (the padding of the key buffer)
      *reinterpret_cast<unsigned short*>(d + (size_t)j * dst.pitch + 2 * (size_t)i) = (unsigned short)vc::reg_key_depth(key[q]);
      if (index) index[(size_t)img * npix + f + q] = vc::reg_key_index(key[q]);
      if (++i == w_d) { i = 0; ++j; }
    }
  }
  u64* c = counters + (size_t)img * vc::kRegCounters + vc::kRegFilled;
  const int filled = (key[0] != vc::kRegEmptyKey) + (key[1] != vc::kRegEmptyKey) + (key[2] != vc::kRegEmptyKey) + (key[3] != vc::kRegEmptyKey);
#pragma unroll
  for (int bit = 0; bit < 3; ++bit) {                          // filled is 0..4: three bit planes, one atomic per wavefront and plane
    const u64 b = __ballot((filled >> bit) & 1);
    if ((threadIdx.x & 63) == 0 && b) atomicAdd(c, (u64)__popcll(b) << bit);
  }
}

// mask (nullable): n x w_s h_s bytes, packed
__global__ __launch_bounds__(256) void k_reg_gather(RegisterPlan p, RegTables t, RegImages depth, const u64* __restrict__ keys, size_t key_stride, RegImages color,
                                                    double occl_tol, int fill, RegImages out, unsigned char* __restrict__ mask) {
  const int ns = p.s.w * p.s.h;
  const int e = blockIdx.x * 256 + threadIdx.x, img = blockIdx.y;
  if (e >= ns) return;
  const int j = e / p.s.w, i = e - j * p.s.w;
  const unsigned value = *reinterpret_cast<const unsigned short*>(depth.p + (size_t)img * depth.stride + (size_t)j * depth.pitch + 2 * (size_t)i);
  bool vis = false;
  int v = fill;
  if (value != 0) {
    double rc[3], x, y, wr;
    int pix;
    const bool okc = load_ray(t.c_xy, t.c_z, (size_t)e, rc);
    if (vc::reg_gather_position(p, value, rc, okc, &x, &y, &pix, &wr) && vc::reg_visible(wr, keys[(size_t)img * key_stride + pix], occl_tol)) {
      vis = true;
      v = min(max((int)floor(vc::reg_bilinear(color.p + (size_t)img * color.stride, color.pitch, p.d.w, p.d.h, x, y) + 0.5), 0), 255);
    }
  }
  out.p[(size_t)img * out.stride + (size_t)j * out.pitch + i] = (unsigned char)v;
  if (mask) mask[(size_t)img * ns + e] = vis ? 1 : 0;
}

__global__ __launch_bounds__(256) void k_reg_points(RegisterPlan p, int n, const double* __restrict__ in, double* __restrict__ out, unsigned char* __restrict__ valid) {
  const int k = blockIdx.x * 256 + threadIdx.x;
  if (k >= n) return;
  double o[3];
  const bool ok = vc::reg_point(p, in[3 * (size_t)k], in[3 * (size_t)k + 1], in[3 * (size_t)k + 2], o);
  const double nan = __builtin_nan("");
  for (int c = 0; c < 3; ++c) out[3 * (size_t)k + c] = ok ? o[c] : nan;
  valid[k] = ok ? 1 : 0;
}

// the arrays of a batch of n images, carved alike from the device allocation and from the pinned one (which has no keys): inputs first and
// outputs last, so that one copy takes [in_depth, in_color) up and one copy brings [counters ...) or [out_color ...) down
struct RegBatch {
  unsigned char* in_depth; unsigned char* in_color;
  u64* keys;
  u64* counters; unsigned char* out_depth; int* out_index;
  unsigned char* out_color; unsigned char* out_mask;
};

}  // namespace

struct vc_registrar {
  int device = 0;
  RegisterPlan p;
  hipStream_t stream = nullptr;
  unsigned char* d_tab = nullptr;
  RegTables tab;
  unsigned char* d_buf = nullptr; unsigned char* h_buf = nullptr;      // grown to the largest batch seen
  RegBatch d, h;
  int cap_images = 0;
  unsigned char* d_pts = nullptr; unsigned char* h_pts = nullptr;      // [in: 3 n doubles | out: 3 n doubles | valid: n bytes]
  int cap_points = 0;
  bool in_flight = false;        // a call left through an error path: the stream may still use the staging buffers
  size_t ns() const { return (size_t)p.s.w * p.s.h; }
  size_t nd() const { return (size_t)p.d.w * p.d.h; }
  size_t key_stride() const { return (nd() + 3) & ~(size_t)3; }
};

namespace {

size_t carve_tables(vc_registrar* r, vch::Carver q) {
  const size_t ns = r->ns(), nl = (size_t)(r->p.s.w + 1) * (r->p.s.h + 1);
  r->tab.c_xy = q.take<double2>(ns); r->tab.c_z = q.take<double>(ns);
  r->tab.l_xy = q.take<double2>(nl); r->tab.l_z = q.take<double>(nl);
  return q.bytes();
}
size_t carve_batch(const vc_registrar* r, int n, bool device, vch::Carver q, RegBatch* b) {
  const size_t ns = r->ns() * n, nd = r->nd() * n;
  b->in_depth = q.take<unsigned char>(2 * ns); b->in_color = q.take<unsigned char>(nd);
  b->keys = device ? q.take<u64>(r->key_stride() * n) : nullptr;
  b->counters = q.take<u64>((size_t)vc::kRegCounters * n); b->out_depth = q.take<unsigned char>(2 * nd); b->out_index = q.take<int>(nd);
  b->out_color = q.take<unsigned char>(ns); b->out_mask = q.take<unsigned char>(ns);
  return q.bytes();
}
bool reserve_images(vc_registrar* r, int n) {
  if (n <= r->cap_images) return true;
  (void)hipStreamSynchronize(r->stream);
  (void)hipFree(r->d_buf);
  if (r->h_buf) (void)hipHostFree(r->h_buf);
  r->d_buf = r->h_buf = nullptr; r->cap_images = 0;
  RegBatch tmp;
  if (hipMalloc((void**)&r->d_buf, carve_batch(r, n, true, vch::Carver(), &tmp)) != hipSuccess ||
      hipHostMalloc((void**)&r->h_buf, carve_batch(r, n, false, vch::Carver(), &tmp), hipHostMallocDefault) != hipSuccess) return false;
  carve_batch(r, n, true, vch::Carver(r->d_buf), &r->d);
  carve_batch(r, n, false, vch::Carver(r->h_buf), &r->h);
  r->cap_images = n;
  return true;
}
size_t points_bytes(int n) { return (size_t)n * 49; }
bool reserve_points(vc_registrar* r, int n) {
  if (n <= r->cap_points) return true;
  (void)hipStreamSynchronize(r->stream);
  (void)hipFree(r->d_pts);
  if (r->h_pts) (void)hipHostFree(r->h_pts);
  r->d_pts = r->h_pts = nullptr; r->cap_points = 0;
  n = (n + 63) & ~63;
  if (hipMalloc((void**)&r->d_pts, points_bytes(n)) != hipSuccess || hipHostMalloc((void**)&r->h_pts, points_bytes(n), hipHostMallocDefault) != hipSuccess) return false;
  r->cap_points = n;
  return true;
}

dim3 grid_of(size_t threads, int n) { return dim3((unsigned)((threads + 255) / 256), (unsigned)n); }
void launch_rays(vc_registrar* r) {
  const size_t total = r->ns() + (size_t)(r->p.s.w + 1) * (r->p.s.h + 1);
  hipLaunchKernelGGL(vc::k_reg_rays, grid_of(total, 1), dim3(256), 0, r->stream, r->p, r->tab, 1);
}
// clear, scatter and (with a destination) resolve of n images whose depth is on the device; counters: n x 8, zeroed here
void launch_depth(vc_registrar* r, int n, RegImages src, bool resolve, RegImages dst, int* index, u64* counters) {
  (void)hipMemsetAsync(r->d.keys, 0xff, r->key_stride() * n * sizeof(u64), r->stream);
  (void)hipMemsetAsync(counters, 0, (size_t)vc::kRegCounters * n * sizeof(u64), r->stream);
  hipLaunchKernelGGL(k_reg_scatter, grid_of(r->ns(), n), dim3(256), 0, r->stream, r->p, r->tab, src, r->d.keys, r->key_stride(), counters);
  if (resolve)
    hipLaunchKernelGGL(k_reg_resolve, grid_of((r->nd() + 3) / 4, n), dim3(256), 0, r->stream, r->p.d.w, (int)r->nd(), r->d.keys, r->key_stride(), dst, index, counters);
}
void launch_gather(vc_registrar* r, int n, RegImages depth, RegImages color, double occl_tol, int fill, RegImages out, unsigned char* mask) {
  hipLaunchKernelGGL(k_reg_gather, grid_of(r->ns(), n), dim3(256), 0, r->stream, r->p, r->tab, depth, r->d.keys, r->key_stride(), color, occl_tol, fill, out, mask);
}
void launch_points(vc_registrar* r, int n) {
  double* in = reinterpret_cast<double*>(r->d_pts); double* out = in + 3 * (size_t)r->cap_points;
  hipLaunchKernelGGL(k_reg_points, grid_of((size_t)n, 1), dim3(256), 0, r->stream, r->p, n, in, out, reinterpret_cast<unsigned char*>(out + 3 * (size_t)r->cap_points));
}

// n images of `width` pixels of `bpp` bytes and `height` rows at p: 16-bit rows and images start on even addresses
bool images_ok(int n, const void* p, int pitch, long long stride, int width, int height, int bpp) {
  if (n > 0 && !p) return false;
  if (pitch < width * bpp || (n > 1 && stride < (long long)pitch * height)) return false;
  return bpp == 1 || ((pitch & 1) == 0 && (stride & 1) == 0 && (reinterpret_cast<size_t>(p) & 1) == 0);
}
// (n = 0 is VC_OK without a launch: nothing else is looked at)
bool depth_args_ok(const vc_registrar* r, int n, const void* src, int src_pitch, long long src_stride, const void* dst, int dst_pitch, long long dst_stride) {
  if (!r || n < 0 || n > kMaxImages) return false;
  return n == 0 || (images_ok(n, src, src_pitch, src_stride, r->p.s.w, r->p.s.h, 2) && images_ok(n, dst, dst_pitch, dst_stride, r->p.d.w, r->p.d.h, 2));
}
void pack_rows(unsigned char* to, const unsigned char* from, int n, int pitch, long long stride, size_t row_bytes, int rows) {
  for (int k = 0; k < n; ++k)
    for (int y = 0; y < rows; ++y) std::memcpy(to + ((size_t)k * rows + y) * row_bytes, from + (size_t)k * stride + (size_t)y * pitch, row_bytes);
}
void unpack_rows(unsigned char* to, const unsigned char* from, int n, int pitch, long long stride, size_t row_bytes, int rows) {
  for (int k = 0; k < n; ++k)
    for (int y = 0; y < rows; ++y) std::memcpy(to + (size_t)k * stride + (size_t)y * pitch, from + ((size_t)k * rows + y) * row_bytes, row_bytes);
}
// a host call starts: the handle's device, no earlier call in flight, room for n images
int begin_call(vc_registrar* r, int n) {
  if (hipSetDevice(r->device) != hipSuccess) return VC_ERR_NO_DEVICE;
  if (r->in_flight) (void)hipStreamSynchronize(r->stream);
  if (n > 0 && !reserve_images(r, n)) return VC_ERR_NO_DEVICE;
  r->in_flight = true;
  return VC_OK;
}

}  // namespace

extern "C" {

int vc_registrar_create(int device, int model_s, const double* params_s, int nparams_s, int w_s, int h_s, const double T_ck_s[7], int model_d, const double* params_d,
                        int nparams_d, int w_d, int h_d, const double T_ck_d[7], double unit_src, double unit_dst, int kind, int splat, vc_registrar** out) {
  double Ts[7], Td[7];
  if (!out || !vc::undist_source_args_ok(model_s, params_s, nparams_s, w_s, h_s) || !vc::undist_source_args_ok(model_d, params_d, nparams_d, w_d, h_d) ||
      !vc::pose_ok(T_ck_s, Ts) || !vc::pose_ok(T_ck_d, Td) || !vc::reg_args_ok(unit_src, unit_dst, kind, splat)) return VC_ERR_BAD_ARG;
  if (vch::open_device(device) != VC_OK) return VC_ERR_NO_DEVICE;
  vc_registrar* r = new vc_registrar;
  r->device = device;
  std::memset(&r->p, 0, sizeof(r->p)); std::memset(&r->d, 0, sizeof(r->d)); std::memset(&r->h, 0, sizeof(r->h));
  vc::reg_cam_fill(&r->p.s, model_s, params_s, nparams_s, w_s, h_s);
  vc::reg_cam_fill(&r->p.d, model_d, params_d, nparams_d, w_d, h_d);
  vc::reg_relative_pose(Ts, Td, r->p.R, r->p.t);
  r->p.unit_src = unit_src; r->p.unit_dst = unit_dst; r->p.kind = kind; r->p.splat = splat;
  if (hipStreamCreate(&r->stream) != hipSuccess || hipMalloc((void**)&r->d_tab, carve_tables(r, vch::Carver())) != hipSuccess) { vc_registrar_destroy(r); return VC_ERR_NO_DEVICE; }
  carve_tables(r, vch::Carver(r->d_tab));
  launch_rays(r);                                      // the tables are built once
  if (hipGetLastError() != hipSuccess || hipStreamSynchronize(r->stream) != hipSuccess) { vc_registrar_destroy(r); return VC_ERR_NO_DEVICE; }
  *out = r;
  return VC_OK;
}
void vc_registrar_destroy(vc_registrar* r) {
  if (!r) return;
  (void)hipSetDevice(r->device);
  if (r->stream) { (void)hipStreamSynchronize(r->stream); (void)hipStreamDestroy(r->stream); }
  (void)hipFree(r->d_tab); (void)hipFree(r->d_buf); (void)hipFree(r->d_pts);
  if (r->h_buf) (void)hipHostFree(r->h_buf);
  if (r->h_pts) (void)hipHostFree(r->h_pts);
  delete r;
}
int vc_register_get(vc_registrar* r, double R[9], double t[3], int size_s[2], int size_d[2], double units[2], int* kind, int* splat) {
  if (!r) return VC_ERR_BAD_ARG;
  if (R) std::memcpy(R, r->p.R, 72);
  if (t) std::memcpy(t, r->p.t, 24);
  if (size_s) { size_s[0] = r->p.s.w; size_s[1] = r->p.s.h; }
  if (size_d) { size_d[0] = r->p.d.w; size_d[1] = r->p.d.h; }
  if (units) { units[0] = r->p.unit_src; units[1] = r->p.unit_dst; }
  if (kind) *kind = r->p.kind;
  if (splat) *splat = r->p.splat;
  return VC_OK;
}
void* vc_register_stream(vc_registrar* r) { return r ? (void*)r->stream : nullptr; }

int vc_register_depth(vc_registrar* r, int n, const unsigned short* src, int src_pitch, long long src_stride, unsigned short* dst, int dst_pitch, long long dst_stride,
                      int* index, long long* counters) {
  if (!depth_args_ok(r, n, src, src_pitch, src_stride, dst, dst_pitch, dst_stride)) return VC_ERR_BAD_ARG;
  if (n == 0) return VC_OK;
  const int rc = begin_call(r, n);
  if (rc != VC_OK) return rc;
  const int ws = r->p.s.w, hs = r->p.s.h, wd = r->p.d.w, hd = r->p.d.h;
  pack_rows(r->h.in_depth, reinterpret_cast<const unsigned char*>(src), n, src_pitch, src_stride, 2 * (size_t)ws, hs);
  if (hipMemcpyAsync(r->d.in_depth, r->h.in_depth, 2 * r->ns() * n, hipMemcpyHostToDevice, r->stream) != hipSuccess) return VC_ERR_NO_DEVICE;
  launch_depth(r, n, RegImages{r->d.in_depth, 2 * ws, 2 * r->ns()}, true, RegImages{r->d.out_depth, 2 * wd, 2 * r->nd()}, index ? r->d.out_index : nullptr, r->d.counters);
  // one download: [counters | depth (| index)] lie behind one another in both allocations
  const unsigned char* end = index ? reinterpret_cast<unsigned char*>(r->d.out_index) + 4 * r->nd() * n : r->d.out_depth + 2 * r->nd() * n;
  if (hipGetLastError() != hipSuccess ||
      hipMemcpyAsync(r->h.counters, r->d.counters, (size_t)(end - reinterpret_cast<unsigned char*>(r->d.counters)), hipMemcpyDeviceToHost, r->stream) != hipSuccess ||
      hipStreamSynchronize(r->stream) != hipSuccess) return VC_ERR_NO_DEVICE;
  r->in_flight = false;
  unpack_rows(reinterpret_cast<unsigned char*>(dst), r->h.out_depth, n, dst_pitch, dst_stride, 2 * (size_t)wd, hd);      // only the pixels: a row's padding is the caller's
  if (index) std::memcpy(index, r->h.out_index, 4 * r->nd() * n);
  if (counters) std::memcpy(counters, r->h.counters, (size_t)vc::kRegCounters * n * 8);
  return VC_OK;
}

int vc_register_depth_device(vc_registrar* r, int n, const unsigned short* d_src, int src_pitch, long long src_stride, unsigned short* d_dst, int dst_pitch,
                             long long dst_stride, int* d_index, long long* d_counters) {
  if (!depth_args_ok(r, n, d_src, src_pitch, src_stride, d_dst, dst_pitch, dst_stride)) return VC_ERR_BAD_ARG;
  if (n == 0) return VC_OK;
  if (hipSetDevice(r->device) != hipSuccess) return VC_ERR_NO_DEVICE;
  if (!reserve_images(r, n)) return VC_ERR_NO_DEVICE;          // (the key buffer: a larger batch than any before waits for the stream and reallocates)
  launch_depth(r, n, RegImages{const_cast<unsigned char*>(reinterpret_cast<const unsigned char*>(d_src)), src_pitch, (size_t)src_stride}, true,
               RegImages{reinterpret_cast<unsigned char*>(d_dst), dst_pitch, (size_t)dst_stride}, d_index, d_counters ? reinterpret_cast<u64*>(d_counters) : r->d.counters);
  return hipGetLastError() == hipSuccess ? VC_OK : VC_ERR_NO_DEVICE;
}

int vc_register_color(vc_registrar* r, int n, const unsigned short* depth, int depth_pitch, long long depth_stride, const unsigned char* color, int color_pitch,
                      long long color_stride, double occl_tol, int fill, unsigned char* out, int out_pitch, long long out_stride, unsigned char* mask) {
  if (!r || n < 0 || n > kMaxImages || !(occl_tol >= 0.0 && occl_tol <= 1e300) || fill < 0 || fill > 255) return VC_ERR_BAD_ARG;
  if (n == 0) return VC_OK;
  if (!images_ok(n, depth, depth_pitch, depth_stride, r->p.s.w, r->p.s.h, 2) || !images_ok(n, color, color_pitch, color_stride, r->p.d.w, r->p.d.h, 1) ||
      !images_ok(n, out, out_pitch, out_stride, r->p.s.w, r->p.s.h, 1)) return VC_ERR_BAD_ARG;
  const int rc = begin_call(r, n);
  if (rc != VC_OK) return rc;
  const int ws = r->p.s.w, hs = r->p.s.h, wd = r->p.d.w, hd = r->p.d.h;
  pack_rows(r->h.in_depth, reinterpret_cast<const unsigned char*>(depth), n, depth_pitch, depth_stride, 2 * (size_t)ws, hs);
  pack_rows(r->h.in_color, color, n, color_pitch, color_stride, (size_t)wd, hd);
  // one upload: [depth | colour], one download: [out (| mask)]
  if (hipMemcpyAsync(r->d.in_depth, r->h.in_depth, (size_t)(r->d.in_color - r->d.in_depth) + r->nd() * n, hipMemcpyHostToDevice, r->stream) != hipSuccess) return VC_ERR_NO_DEVICE;
  const RegImages d_depth{r->d.in_depth, 2 * ws, 2 * r->ns()};
  launch_depth(r, n, d_depth, false, RegImages{nullptr, 0, 0}, nullptr, r->d.counters);
  launch_gather(r, n, d_depth, RegImages{r->d.in_color, wd, r->nd()}, occl_tol, fill, RegImages{r->d.out_color, ws, r->ns()}, mask ? r->d.out_mask : nullptr);
  const size_t down = mask ? (size_t)(r->d.out_mask - r->d.out_color) + r->ns() * n : r->ns() * n;
  if (hipGetLastError() != hipSuccess || hipMemcpyAsync(r->h.out_color, r->d.out_color, down, hipMemcpyDeviceToHost, r->stream) != hipSuccess ||
      hipStreamSynchronize(r->stream) != hipSuccess) return VC_ERR_NO_DEVICE;
  r->in_flight = false;
  unpack_rows(out, r->h.out_color, n, out_pitch, out_stride, (size_t)ws, hs);
  if (mask) std::memcpy(mask, r->h.out_mask, r->ns() * n);
  return VC_OK;
}

int vc_register_points(vc_registrar* r, int n, const double* in, double* out, unsigned char* valid) {
  if (!r || n < 0 || (n > 0 && (!in || !out))) return VC_ERR_BAD_ARG;
  if (n == 0) return VC_OK;
  if (hipSetDevice(r->device) != hipSuccess) return VC_ERR_NO_DEVICE;
  if (r->in_flight) (void)hipStreamSynchronize(r->stream);
  if (!reserve_points(r, n)) return VC_ERR_NO_DEVICE;
  r->in_flight = true;
  const size_t cap = (size_t)r->cap_points;
  std::memcpy(r->h_pts, in, (size_t)n * 24);
  if (hipMemcpyAsync(r->d_pts, r->h_pts, (size_t)n * 24, hipMemcpyHostToDevice, r->stream) != hipSuccess) return VC_ERR_NO_DEVICE;
  launch_points(r, n);
  // results: out (3 n doubles at 24 cap) and valid (n bytes at 48 cap) -- two copies, one synchronisation
  if (hipGetLastError() != hipSuccess ||
      hipMemcpyAsync(r->h_pts + 24 * cap, r->d_pts + 24 * cap, (size_t)n * 24, hipMemcpyDeviceToHost, r->stream) != hipSuccess ||
      hipMemcpyAsync(r->h_pts + 48 * cap, r->d_pts + 48 * cap, (size_t)n, hipMemcpyDeviceToHost, r->stream) != hipSuccess ||
      hipStreamSynchronize(r->stream) != hipSuccess) return VC_ERR_NO_DEVICE;
  r->in_flight = false;
  std::memcpy(out, r->h_pts + 24 * cap, (size_t)n * 24);
  if (valid) std::memcpy(valid, r->h_pts + 48 * cap, (size_t)n);
  return VC_OK;
}

int vc_time_register(vc_registrar* r, int n_images, int reps, double out_ms[4]) {
  if (!r || n_images < 1 || n_images > kMaxImages || reps < 1 || !out_ms) return VC_ERR_BAD_ARG;
  if (hipSetDevice(r->device) != hipSuccess) return VC_ERR_NO_DEVICE;
  if (r->in_flight) (void)hipStreamSynchronize(r->stream);
  if (!reserve_images(r, n_images) || !reserve_points(r, kTimePoints)) return VC_ERR_NO_DEVICE;
  r->in_flight = true;
  // device-resident inputs: a slanted surface of 1000 .. 2499 counts, a grey ramp, a lattice of points over the source image
  const int ws = r->p.s.w, hs = r->p.s.h, wd = r->p.d.w;
  unsigned short* hd = reinterpret_cast<unsigned short*>(r->h.in_depth);
  for (int k = 0; k < n_images; ++k)
    for (int j = 0; j < hs; ++j)
      for (int i = 0; i < ws; ++i) hd[((size_t)k * hs + j) * ws + i] = (unsigned short)(1000 + (3 * i + 5 * j + 11 * k) % 1500);
  for (size_t k = 0; k < r->nd() * n_images; ++k) r->h.in_color[k] = (unsigned char)((k * 7) & 255);
  double* hp = reinterpret_cast<double*>(r->h_pts);
  const int side = 256;
  for (int k = 0; k < kTimePoints; ++k) {
    hp[3 * k] = (ws - 1.0) * (k % side) / (side - 1.0);
    hp[3 * k + 1] = (hs - 1.0) * (k / side) / (side - 1.0);
    hp[3 * k + 2] = 1000.0 + (k % 1500);
  }
  if (hipMemcpyAsync(r->d.in_depth, r->h.in_depth, (size_t)(r->d.in_color - r->d.in_depth) + r->nd() * n_images, hipMemcpyHostToDevice, r->stream) != hipSuccess ||
      hipMemcpyAsync(r->d_pts, r->h_pts, (size_t)kTimePoints * 24, hipMemcpyHostToDevice, r->stream) != hipSuccess) return VC_ERR_NO_DEVICE;
  const RegImages d_depth{r->d.in_depth, 2 * ws, 2 * r->ns()};
  for (int what = 0; what < 4; ++what) {
    auto launch = [&]() {                              // (the tables a launch rewrites are the same tables; the gather reads the keys of the scatter before it)
      if (what == 0) launch_rays(r);
      else if (what == 1) launch_depth(r, n_images, d_depth, true, RegImages{r->d.out_depth, 2 * wd, 2 * r->nd()}, r->d.out_index, r->d.counters);
      else if (what == 2) launch_gather(r, n_images, d_depth, RegImages{r->d.in_color, wd, r->nd()}, 0.0, 0, RegImages{r->d.out_color, ws, r->ns()}, r->d.out_mask);
      else launch_points(r, kTimePoints);
    };
    const int rc = vch::time_back_to_back(r->stream, reps, launch, &out_ms[what]);
    if (rc != VC_OK) return rc;
  }
  r->in_flight = false;
  return VC_OK;
}

}  // extern "C"
