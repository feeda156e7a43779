// vc_depthcal.hip -- the range error of a depth camera measured against the calibration target, on the GPU: every depth pixel that looks at
// the board (the plane z_w = 0) compared with the distance the calibration says it should have reported, binned into image cells, fitted
// on the host from the sums, and the correction applied to depth images.  Definitions: include/vicalib_amd.h; the arithmetic: vc_depthcal.hpp.
//
//   k_reg_rays        (vc_reg_rays.hpp, the registrar's) built once at create: the ray of every pixel centre
//   k_dc_accumulate   the hot path.  A workgroup owns one CHUNK of one cell of one frame: the cell's pixels in row-major order cut into
//                     pieces of kChunk; lane t takes pixels t, t + 256, ...  The nine terms are reduced over the wavefront by the xor
//                     butterfly (wave_allsum), over the four wavefronts through LDS in wavefront order, and stored as one record per
//                     (frame, chunk): no floating-point atomic anywhere, so the bits depend on the image size and the bins only.  Rules are
//                     counted by ballot, one integer atomicAdd per wavefront and rule.  The grid is (chunks rounded up to 8) x frames:
//                     a chunk's workgroups of all frames of the batch then share one XCD, whose L2 keeps its eighth of the ray table over
//                     the batch.
//   k_dc_fold         one thread per (cell, sum): the records added into the running sums in (frame, chunk) order -- a batch of 8, 3 + 5
//                     and eight single calls perform the same additions in the same order
//   k_dc_expected     one thread per pixel: the expected value and the rule
//   k_dc_apply        four consecutive pixels per thread, one 8-byte load and store where the quad is whole
// No CPU fallback: vc_depthcal_create fails with VC_ERR_NO_DEVICE without a HIP device.
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstring>
#include <vector>
#include "../../include/vicalib_amd.h"
#include "vc_hostutil.hpp"
#include "vc_kutil.hpp"
#include "vc_reg_rays.hpp"
#include "vc_depthcal.hpp"

namespace {

using vc::DepthCalPlan;
using vc::DcFrame;
using vc::DcPoly;
typedef unsigned long long u64;
constexpr int kChunk = 1024;                           // pixels of a chunk: four per lane
constexpr int kMaxImages = 65535;                      // (the image index is the grid's y)

struct DcCellRec { int i0, cw, j0, ch, chunk0, nchunks; };      // the cell's rectangle of pixels and its chunks
struct DcChunkRec { int cell, first; };                         // first: the chunk's first pixel in the cell's row-major order
// a batch of packed 16-bit images on the device: rows 2 w bytes apart, images `stride` bytes apart (a multiple of 8)
struct DcImages { unsigned char* p; size_t stride; };

__global__ __launch_bounds__(256) void k_dc_accumulate(DepthCalPlan p, const double2* __restrict__ c_xy, const double* __restrict__ c_z, DcImages src,
                                                       const DcFrame* __restrict__ frames, const DcCellRec* __restrict__ cells, const DcChunkRec* __restrict__ chunks,
                                                       int nchunks, double* __restrict__ partial, u64* __restrict__ counters) {
  const int chunk = blockIdx.x, img = blockIdx.y;
  if (chunk >= nchunks) return;                        // (the grid's padding: the whole workgroup leaves)
  const DcChunkRec ck = chunks[chunk];
  const DcCellRec cl = cells[ck.cell];
  const DcFrame& f = frames[img];
  const int count = cl.cw * cl.ch;
  const unsigned char* im = src.p + (size_t)img * src.stride;
  double acc[vc::kDcSums];
  unsigned cnt[vc::kDcCounters];
#pragma unroll
  for (int t = 0; t < vc::kDcSums; ++t) acc[t] = 0.0;
#pragma unroll
  for (int r = 0; r < vc::kDcCounters; ++r) cnt[r] = 0;
#pragma unroll
  for (int q = 0; q < kChunk / 256; ++q) {
    const int e = ck.first + q * 256 + (int)threadIdx.x;
    int rule = -1;                                     // (a lane beyond the cell counts nowhere)
    if (e < count) {
      const int jj = e / cl.cw, i = cl.i0 + (e - jj * cl.cw), j = cl.j0 + jj;
      const size_t k = (size_t)j * p.w + i;            // below w h: the cell's rectangle lies in the image
      const unsigned value = *reinterpret_cast<const unsigned short*>(im + 2 * k);
      rule = vc::kDcDropZero;
      if (value != 0) {
        double ray[3], y;
        const bool ok = vc::load_ray(c_xy, c_z, k, ray);
        rule = vc::dc_expected(p, f, ray, ok, true, value, &y);
        if (rule == vc::kDcUsed) {
          double t[vc::kDcSums];
          vc::dc_terms(p, value, y, t);
#pragma unroll
          for (int s = 0; s < vc::kDcSums; ++s) acc[s] += t[s];
        }
      }
    }
#pragma unroll
    for (int r = 0; r < vc::kDcCounters; ++r) cnt[r] += (unsigned)__popcll(__ballot(rule == r));
  }
  __shared__ double s_part[4][vc::kDcSums];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
#pragma unroll
  for (int t = 0; t < vc::kDcSums; ++t) {
    const double v = vc::wave_allsum(acc[t]);
    if (lane == 0) s_part[wave][t] = v;
  }
  __syncthreads();
  if (threadIdx.x < vc::kDcSums)
    partial[((size_t)img * nchunks + chunk) * vc::kDcSums + threadIdx.x] =
        ((s_part[0][threadIdx.x] + s_part[1][threadIdx.x]) + s_part[2][threadIdx.x]) + s_part[3][threadIdx.x];
  if (lane == 0) {
    u64* c = counters + (size_t)img * vc::kDcCounters;
#pragma unroll
    for (int r = 0; r < vc::kDcCounters; ++r)
      if (cnt[r]) atomicAdd(c + r, (u64)cnt[r]);
  }
}

// running: cells x 9
__global__ __launch_bounds__(256) void k_dc_fold(const DcCellRec* __restrict__ cells, int ncells, int n, int nchunks, const double* __restrict__ partial,
                                                 double* __restrict__ running) {
  const int k = blockIdx.x * 256 + threadIdx.x;
  if (k >= ncells * vc::kDcSums) return;
  const int cell = k / vc::kDcSums, t = k - cell * vc::kDcSums;
  const int c0 = cells[cell].chunk0, c1 = c0 + cells[cell].nchunks;
  double r = running[k];
  for (int img = 0; img < n; ++img) {
    const double* q = partial + (size_t)img * nchunks * vc::kDcSums + t;
#pragma unroll 8
    for (int c = c0; c < c1; ++c) r += q[(size_t)c * vc::kDcSums];
  }
  running[k] = r;
}

// y: n x npix doubles, rule: n x npix bytes
__global__ __launch_bounds__(256) void k_dc_expected(DepthCalPlan p, const double2* __restrict__ c_xy, const double* __restrict__ c_z, DcImages src, int has_depth,
                                                     const DcFrame* __restrict__ frames, double* __restrict__ y, unsigned char* __restrict__ rule) {
  const int npix = p.w * p.h;
  const int e = blockIdx.x * 256 + threadIdx.x, img = blockIdx.y;
  if (e >= npix) return;
  const unsigned value = has_depth ? *reinterpret_cast<const unsigned short*>(src.p + (size_t)img * src.stride + 2 * (size_t)e) : 0u;
  double ray[3], yv;
  const bool ok = vc::load_ray(c_xy, c_z, (size_t)e, ray);
  const int code = vc::dc_expected(p, frames[img], ray, ok, has_depth != 0, value, &yv);
  y[(size_t)img * npix + e] = yv;
  rule[(size_t)img * npix + e] = (unsigned char)code;
}

// counters: n x 3 (zeros in, corrected, out of range); a, b: cells
__global__ __launch_bounds__(256) void k_dc_apply(DepthCalPlan p, DcPoly poly, const double* __restrict__ a, const double* __restrict__ b, int interp, DcImages src,
                                                  DcImages dst, u64* __restrict__ counters) {
  const int npix = p.w * p.h;
  const int f = (blockIdx.x * 256 + threadIdx.x) << 2, img = blockIdx.y;
  int n_zero = 0, n_done = 0, n_out = 0;
  if (f < npix) {                                      // (an image starts on a multiple of 8 bytes: so does every quad)
    const unsigned char* s = src.p + (size_t)img * src.stride + 2 * (size_t)f;
    unsigned char* d = dst.p + (size_t)img * dst.stride + 2 * (size_t)f;
    const bool whole = f + 3 < npix;
    unsigned v[4] = {0, 0, 0, 0};
    if (whole) {
      const uint2 raw = *reinterpret_cast<const uint2*>(s);
      v[0] = raw.x & 0xffffu; v[1] = raw.x >> 16; v[2] = raw.y & 0xffffu; v[3] = raw.y >> 16;
    } else {
#pragma unroll
      for (int q = 0; q < 3; ++q)
        if (f + q < npix) v[q] = reinterpret_cast<const unsigned short*>(s)[q];
    }
    int j = f / p.w, i = f - j * p.w;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      if (f + q < npix) {
        int what = 0;
        if (v[q] != 0) {
          double A, B;
          vc::dc_cell_terms(p, a, b, interp, i, j, &A, &B);
          v[q] = vc::dc_apply(poly, v[q], A, B, &what);
        }
        n_zero += what == 0; n_done += what == 1; n_out += what == 2;
        if (++i == p.w) { i = 0; ++j; }
      }
    }
    if (whole) *reinterpret_cast<uint2*>(d) = make_uint2(v[0] | (v[1] << 16), v[2] | (v[3] << 16));
    else {
#pragma unroll
      for (int q = 0; q < 3; ++q)
        if (f + q < npix) reinterpret_cast<unsigned short*>(d)[q] = (unsigned short)v[q];
    }
  }
  u64* c = counters + (size_t)img * 3;
#pragma unroll
  for (int what = 0; what < 3; ++what) {
    const int m_what = what == 0 ? n_zero : what == 1 ? n_done : n_out;
#pragma unroll
    for (int bit = 0; bit < 3; ++bit) {                // a count is 0..4: three bit planes, one atomic per wavefront and plane
      const u64 m = __ballot((m_what >> bit) & 1);
      if ((threadIdx.x & 63) == 0 && m) atomicAdd(c + what, (u64)__popcll(m) << bit);
    }
  }
}

}  // namespace

struct vc_depthcal {
  int device = 0;
  vc::RegisterPlan cam;                                // the depth camera as the registrar's source (what the ray kernel reads)
  DepthCalPlan p;
  double T_ck[7];
  hipStream_t stream = nullptr;
  unsigned char* d_fix = nullptr;                      // everything that lives as long as the handle
  vc::RegTables tab;
  DcCellRec* d_cells = nullptr; DcChunkRec* d_chunks = nullptr;
  double* d_running = nullptr; double* d_a = nullptr; double* d_b = nullptr;
  int ncells = 0, nchunks = 0;
  unsigned char* d_buf = nullptr; unsigned char* h_buf = nullptr;      // staging, grown to the largest call seen
  size_t cap_d = 0, cap_h = 0;
  bool in_flight = false;
  long long counters[vc::kDcCounters] = {0, 0, 0, 0, 0, 0, 0, 0};
  long long n_frames = 0;
  // the fit: from the sums (invalidated by add and clear) or set by the caller
  bool have_fit = false, fit_from_sums = false;
  int degree = 0;
  DcPoly poly;
  std::vector<double> a, b, sums;
  std::vector<int> status;
  double rms[3] = {0, 0, 0};
  size_t npix() const { return (size_t)p.w * p.h; }
  size_t img_stride() const { return (2 * npix() + 7) & ~(size_t)7; }
};

namespace {

size_t carve_fixed(vc_depthcal* d, vch::Carver q) {
  d->tab.c_xy = q.take<double2>(d->npix()); d->tab.c_z = q.take<double>(d->npix());
  d->tab.l_xy = nullptr; d->tab.l_z = nullptr;
  d->d_cells = q.take<DcCellRec>(d->ncells); d->d_chunks = q.take<DcChunkRec>(d->nchunks);
  d->d_running = q.take<double>((size_t)d->ncells * vc::kDcSums);
  d->d_a = q.take<double>(d->ncells); d->d_b = q.take<double>(d->ncells);
  return q.bytes();
}
bool reserve(vc_depthcal* d, size_t bytes_d, size_t bytes_h) {
  if (bytes_d <= d->cap_d && bytes_h <= d->cap_h) return true;
  (void)hipStreamSynchronize(d->stream);
  (void)hipFree(d->d_buf);
  if (d->h_buf) (void)hipHostFree(d->h_buf);
  d->d_buf = d->h_buf = nullptr; d->cap_d = d->cap_h = 0;
  bytes_d = bytes_d > d->cap_d ? bytes_d : d->cap_d; bytes_h = bytes_h > d->cap_h ? bytes_h : d->cap_h;
  if (hipMalloc((void**)&d->d_buf, bytes_d) != hipSuccess || hipHostMalloc((void**)&d->h_buf, bytes_h, hipHostMallocDefault) != hipSuccess) return false;
  d->cap_d = bytes_d; d->cap_h = bytes_h;
  return true;
}
// the arrays of a call over n images, carved alike from the device staging and the pinned one: what goes up first ([frames | depth]), what
// comes down last
struct DcBatch {
  DcFrame* frames; unsigned char* depth;               // up
  double* partial;                                     // device only
  u64* counters; unsigned char* out_depth;             // down: add [counters], apply [counters | out_depth]
  double* y; unsigned char* rule;                      // down: expected [y | rule]
};
enum { kCallAdd = 0, kCallExpected = 1, kCallApply = 2 };
size_t carve_batch(const vc_depthcal* d, int n, int call, bool device, vch::Carver q, DcBatch* b) {
  std::memset(b, 0, sizeof(*b));
  b->frames = q.take<DcFrame>(n); b->depth = q.take<unsigned char>(d->img_stride() * n);
  if (call == kCallAdd) {
    if (device) b->partial = q.take<double>((size_t)n * d->nchunks * vc::kDcSums);
    b->counters = q.take<u64>((size_t)vc::kDcCounters * n);
  } else if (call == kCallExpected) {
    b->y = q.take<double>(d->npix() * n); b->rule = q.take<unsigned char>(d->npix() * n);
  } else {
    b->counters = q.take<u64>((size_t)3 * n); b->out_depth = q.take<unsigned char>(d->img_stride() * n);
  }
  return q.bytes();
}
// a host call starts: the handle's device, no earlier call in flight, staging for the call
int begin_call(vc_depthcal* d, int n, int call, DcBatch* dev, DcBatch* host) {
  if (hipSetDevice(d->device) != hipSuccess) return VC_ERR_NO_DEVICE;
  if (d->in_flight) (void)hipStreamSynchronize(d->stream);
  DcBatch tmp;
  if (!reserve(d, carve_batch(d, n, call, true, vch::Carver(), &tmp), carve_batch(d, n, call, false, vch::Carver(), &tmp))) return VC_ERR_NO_DEVICE;
  carve_batch(d, n, call, true, vch::Carver(d->d_buf), dev);
  carve_batch(d, n, call, false, vch::Carver(d->h_buf), host);
  d->in_flight = true;
  return VC_OK;
}

dim3 grid_of(size_t threads, int n) { return dim3((unsigned)((threads + 255) / 256), (unsigned)n); }
void launch_rays(vc_depthcal* d) { hipLaunchKernelGGL(vc::k_reg_rays, grid_of(d->npix(), 1), dim3(256), 0, d->stream, d->cam, d->tab, 0); }
// n frames whose images and records are on the device: accumulate (counters n x 8, zeroed here), fold into `running`
void launch_add(vc_depthcal* d, int n, DcImages src, const DcFrame* frames, double* partial, u64* counters, double* running) {
  (void)hipMemsetAsync(counters, 0, (size_t)vc::kDcCounters * n * sizeof(u64), d->stream);
  hipLaunchKernelGGL(k_dc_accumulate, dim3((unsigned)((d->nchunks + 7) & ~7), (unsigned)n), dim3(256), 0, d->stream, d->p, d->tab.c_xy, d->tab.c_z, src, frames, d->d_cells,
                     d->d_chunks, d->nchunks, partial, counters);
  hipLaunchKernelGGL(k_dc_fold, grid_of((size_t)d->ncells * vc::kDcSums, 1), dim3(256), 0, d->stream, d->d_cells, d->ncells, n, d->nchunks, partial, running);
}
void launch_apply(vc_depthcal* d, int n, const DcPoly& poly, const double* a, const double* b, int interp, DcImages src, DcImages dst, u64* counters) {
  (void)hipMemsetAsync(counters, 0, (size_t)3 * n * sizeof(u64), d->stream);
  hipLaunchKernelGGL(k_dc_apply, grid_of((d->npix() + 3) / 4, n), dim3(256), 0, d->stream, d->p, poly, a, b, interp, src, dst, counters);
}

// n images of 16-bit rows at p (the registrar's rules): rows and images start on even addresses
bool images_ok(int n, const void* p, int pitch, long long stride, int width, int height) {
  if (n > 0 && !p) return false;
  if (pitch < width * 2 || (n > 1 && stride < (long long)pitch * height)) return false;
  return (pitch & 1) == 0 && (stride & 1) == 0 && (reinterpret_cast<size_t>(p) & 1) == 0;
}
void pack_images(const vc_depthcal* d, unsigned char* to, const unsigned char* from, int n, int pitch, long long stride) {
  const size_t row = 2 * (size_t)d->p.w;
  for (int k = 0; k < n; ++k)
    for (int y = 0; y < d->p.h; ++y) std::memcpy(to + (size_t)k * d->img_stride() + y * row, from + (size_t)k * stride + (size_t)y * pitch, row);
}
// the frames' records from their poses; false: a pose that is not finite or not of unit length
bool fill_frames(const vc_depthcal* d, int n, const double* T_wk, DcFrame* out) {
  for (int k = 0; k < n; ++k) {
    double T[7];
    if (!vc::pose_ok(T_wk + 7 * (size_t)k, T)) return false;
    vc::dc_frame(d->T_ck, T, &out[k]);
  }
  return true;
}
void drop_fit_from_sums(vc_depthcal* d) { if (d->fit_from_sums) d->have_fit = d->fit_from_sums = false; }
int upload_fit(vc_depthcal* d) {
  if (hipSetDevice(d->device) != hipSuccess) return VC_ERR_NO_DEVICE;
  if (hipMemcpy(d->d_a, d->a.data(), d->ncells * sizeof(double), hipMemcpyHostToDevice) != hipSuccess ||
      hipMemcpy(d->d_b, d->b.data(), d->ncells * sizeof(double), hipMemcpyHostToDevice) != hipSuccess) return VC_ERR_NO_DEVICE;
  return VC_OK;
}
int fetch_sums(vc_depthcal* d) {
  if (hipSetDevice(d->device) != hipSuccess) return VC_ERR_NO_DEVICE;
  if (d->in_flight) { (void)hipStreamSynchronize(d->stream); d->in_flight = false; }
  d->sums.resize((size_t)d->ncells * vc::kDcSums);
  return hipMemcpy(d->sums.data(), d->d_running, d->sums.size() * sizeof(double), hipMemcpyDeviceToHost) == hipSuccess ? VC_OK : VC_ERR_NO_DEVICE;
}

}  // namespace

extern "C" {

int vc_depthcal_create(int device, int model, const double* params, int nparams, int w, int h, const double T_ck[7], double unit, int kind, const double rect[4],
                       int bins_x, int bins_y, double v_ref, double min_cos, double max_dev, vc_depthcal** out) {
  double T[7];
  if (!out || !vc::undist_source_args_ok(model, params, nparams, w, h) || !vc::pose_ok(T_ck, T) ||
      !vc::dc_args_ok(unit, kind, rect, bins_x, bins_y, v_ref, min_cos, max_dev)) return VC_ERR_BAD_ARG;
  if (vch::open_device(device) != VC_OK) return VC_ERR_NO_DEVICE;
  vc_depthcal* d = new vc_depthcal;
  d->device = device;
  std::memset(&d->cam, 0, sizeof(d->cam)); std::memset(&d->p, 0, sizeof(d->p));
  vc::reg_cam_fill(&d->cam.s, model, params, nparams, w, h);
  d->cam.kind = kind; d->cam.splat = vc::kRegNearest; d->cam.unit_src = d->cam.unit_dst = unit;
  std::memcpy(d->T_ck, T, sizeof(T));
  DepthCalPlan& p = d->p;
  p.w = w; p.h = h; p.kind = kind; p.bins_x = bins_x; p.bins_y = bins_y; p.unit = unit; p.v_ref = v_ref; p.min_cos = min_cos; p.max_dev = max_dev;
  std::memcpy(p.rect, rect, 32);
  d->poly.c[0] = d->poly.c[1] = d->poly.c[2] = 0.0; d->poly.v_ref = v_ref;
  // the cells' rectangles and their chunks: cell (cx, cy) holds the pixels report_cell sends there
  d->ncells = bins_x * bins_y;
  std::vector<DcCellRec> cells(d->ncells);
  std::vector<DcChunkRec> chunks;
  for (int cy = 0; cy < bins_y; ++cy)
    for (int cx = 0; cx < bins_x; ++cx) {
      DcCellRec& c = cells[cy * bins_x + cx];
      c.i0 = vc::dc_cell_begin(cx, bins_x, w); c.cw = vc::dc_cell_begin(cx + 1, bins_x, w) - c.i0;
      c.j0 = vc::dc_cell_begin(cy, bins_y, h); c.ch = vc::dc_cell_begin(cy + 1, bins_y, h) - c.j0;
      c.chunk0 = (int)chunks.size(); c.nchunks = (c.cw * c.ch + kChunk - 1) / kChunk;
      for (int k = 0; k < c.nchunks; ++k) chunks.push_back(DcChunkRec{cy * bins_x + cx, k * kChunk});
    }
  d->nchunks = (int)chunks.size();
  d->a.assign(d->ncells, 0.0); d->b.assign(d->ncells, 0.0); d->status.assign(d->ncells, vc::kDcTooFew);
  if (hipStreamCreate(&d->stream) != hipSuccess || hipMalloc((void**)&d->d_fix, carve_fixed(d, vch::Carver())) != hipSuccess) { vc_depthcal_destroy(d); return VC_ERR_NO_DEVICE; }
  carve_fixed(d, vch::Carver(d->d_fix));
  bool ok = hipMemcpyAsync(d->d_cells, cells.data(), cells.size() * sizeof(DcCellRec), hipMemcpyHostToDevice, d->stream) == hipSuccess &&
            hipMemcpyAsync(d->d_chunks, chunks.data(), chunks.size() * sizeof(DcChunkRec), hipMemcpyHostToDevice, d->stream) == hipSuccess &&
            hipMemsetAsync(d->d_running, 0, (size_t)d->ncells * vc::kDcSums * sizeof(double), d->stream) == hipSuccess;
  launch_rays(d);                                      // the table is built once
  ok = ok && hipGetLastError() == hipSuccess && hipStreamSynchronize(d->stream) == hipSuccess;      // (the vectors above live until here)
  if (!ok) { vc_depthcal_destroy(d); return VC_ERR_NO_DEVICE; }
  *out = d;
  return VC_OK;
}
void vc_depthcal_destroy(vc_depthcal* d) {
  if (!d) return;
  (void)hipSetDevice(d->device);
  if (d->stream) { (void)hipStreamSynchronize(d->stream); (void)hipStreamDestroy(d->stream); }
  (void)hipFree(d->d_fix); (void)hipFree(d->d_buf);
  if (d->h_buf) (void)hipHostFree(d->h_buf);
  delete d;
}
int vc_depthcal_get(vc_depthcal* d, int size[2], int bins[2], double* unit, int* kind, double rect[4], double* v_ref, double* min_cos, double* max_dev, double R_ck[9],
                    double t_ck[3]) {
  if (!d) return VC_ERR_BAD_ARG;
  if (size) { size[0] = d->p.w; size[1] = d->p.h; }
  if (bins) { bins[0] = d->p.bins_x; bins[1] = d->p.bins_y; }
  if (unit) *unit = d->p.unit;
  if (kind) *kind = d->p.kind;
  if (rect) std::memcpy(rect, d->p.rect, 32);
  if (v_ref) *v_ref = d->p.v_ref;
  if (min_cos) *min_cos = d->p.min_cos;
  if (max_dev) *max_dev = d->p.max_dev;
  if (R_ck) vc::quat_to_R(d->T_ck, R_ck);
  if (t_ck) std::memcpy(t_ck, d->T_ck + 4, 24);
  return VC_OK;
}
int vc_depthcal_clear(vc_depthcal* d) {
  if (!d) return VC_ERR_BAD_ARG;
  if (hipSetDevice(d->device) != hipSuccess) return VC_ERR_NO_DEVICE;
  if (hipMemsetAsync(d->d_running, 0, (size_t)d->ncells * vc::kDcSums * sizeof(double), d->stream) != hipSuccess ||
      hipStreamSynchronize(d->stream) != hipSuccess) return VC_ERR_NO_DEVICE;
  d->in_flight = false;
  std::memset(d->counters, 0, sizeof(d->counters));
  d->n_frames = 0;
  drop_fit_from_sums(d);
  return VC_OK;
}

int vc_depthcal_add(vc_depthcal* d, int n, const unsigned short* depth, int pitch, long long stride, const double* T_wk, long long* counters) {
  if (!d || n < 0 || n > kMaxImages) return VC_ERR_BAD_ARG;
  if (n == 0) return VC_OK;
  if (!images_ok(n, depth, pitch, stride, d->p.w, d->p.h) || !T_wk) return VC_ERR_BAD_ARG;
  std::vector<DcFrame> frames(n);
  if (!fill_frames(d, n, T_wk, frames.data())) return VC_ERR_BAD_ARG;      // (before anything is added)
  DcBatch dev, host;
  const int rc = begin_call(d, n, kCallAdd, &dev, &host);
  if (rc != VC_OK) return rc;
  std::memcpy(host.frames, frames.data(), (size_t)n * sizeof(DcFrame));
  pack_images(d, host.depth, reinterpret_cast<const unsigned char*>(depth), n, pitch, stride);
  // one upload: [frames | depth]
  const size_t up = (size_t)(dev.depth - reinterpret_cast<unsigned char*>(dev.frames)) + d->img_stride() * n;
  if (hipMemcpyAsync(dev.frames, host.frames, up, hipMemcpyHostToDevice, d->stream) != hipSuccess) return VC_ERR_NO_DEVICE;
  drop_fit_from_sums(d);
  launch_add(d, n, DcImages{dev.depth, d->img_stride()}, dev.frames, dev.partial, dev.counters, d->d_running);
  if (hipGetLastError() != hipSuccess ||
      hipMemcpyAsync(host.counters, dev.counters, (size_t)vc::kDcCounters * n * 8, hipMemcpyDeviceToHost, d->stream) != hipSuccess ||
      hipStreamSynchronize(d->stream) != hipSuccess) return VC_ERR_NO_DEVICE;
  d->in_flight = false;
  for (int k = 0; k < n; ++k)
    for (int r = 0; r < vc::kDcCounters; ++r) d->counters[r] += (long long)host.counters[(size_t)k * vc::kDcCounters + r];
  d->n_frames += n;
  if (counters) std::memcpy(counters, host.counters, (size_t)vc::kDcCounters * n * 8);
  return VC_OK;
}

int vc_depthcal_expected(vc_depthcal* d, int n, const double* T_wk, const unsigned short* depth, int pitch, long long stride, double* y, unsigned char* rule) {
  if (!d || n < 0 || n > kMaxImages) return VC_ERR_BAD_ARG;
  if (n == 0) return VC_OK;
  if (!T_wk || !y || !rule || (depth && !images_ok(n, depth, pitch, stride, d->p.w, d->p.h))) return VC_ERR_BAD_ARG;
  std::vector<DcFrame> frames(n);
  if (!fill_frames(d, n, T_wk, frames.data())) return VC_ERR_BAD_ARG;
  DcBatch dev, host;
  const int rc = begin_call(d, n, kCallExpected, &dev, &host);
  if (rc != VC_OK) return rc;
  std::memcpy(host.frames, frames.data(), (size_t)n * sizeof(DcFrame));
  size_t up = (size_t)n * sizeof(DcFrame);
  if (depth) {
    pack_images(d, host.depth, reinterpret_cast<const unsigned char*>(depth), n, pitch, stride);
    up = (size_t)(dev.depth - reinterpret_cast<unsigned char*>(dev.frames)) + d->img_stride() * n;
  }
  if (hipMemcpyAsync(dev.frames, host.frames, up, hipMemcpyHostToDevice, d->stream) != hipSuccess) return VC_ERR_NO_DEVICE;
  hipLaunchKernelGGL(k_dc_expected, grid_of(d->npix(), n), dim3(256), 0, d->stream, d->p, d->tab.c_xy, d->tab.c_z, DcImages{dev.depth, d->img_stride()}, depth ? 1 : 0,
                     dev.frames, dev.y, dev.rule);
  // one download: [y | rule] lie behind one another in both allocations
  const size_t down = (size_t)(dev.rule - reinterpret_cast<unsigned char*>(dev.y)) + d->npix() * n;
  if (hipGetLastError() != hipSuccess || hipMemcpyAsync(host.y, dev.y, down, hipMemcpyDeviceToHost, d->stream) != hipSuccess ||
      hipStreamSynchronize(d->stream) != hipSuccess) return VC_ERR_NO_DEVICE;
  d->in_flight = false;
  std::memcpy(y, host.y, d->npix() * n * sizeof(double));
  std::memcpy(rule, host.rule, d->npix() * n);
  return VC_OK;
}

int vc_depthcal_sums(vc_depthcal* d, double* sums, double totals[9], long long counters[8], long long* n_frames) {
  if (!d) return VC_ERR_BAD_ARG;
  if (sums || totals) {
    const int rc = fetch_sums(d);
    if (rc != VC_OK) return rc;
    if (sums) std::memcpy(sums, d->sums.data(), d->sums.size() * sizeof(double));
    if (totals)
      for (int t = 0; t < vc::kDcSums; ++t) {                      // the cells in their order
        totals[t] = 0.0;
        for (int k = 0; k < d->ncells; ++k) totals[t] += d->sums[(size_t)k * vc::kDcSums + t];
      }
  }
  if (counters) std::memcpy(counters, d->counters, sizeof(d->counters));
  if (n_frames) *n_frames = d->n_frames;
  return VC_OK;
}

int vc_depthcal_fit(vc_depthcal* d, int degree, int min_count, double min_spread) {
  if (!d || degree < 0 || degree > 2 || min_count < 1 || !(min_spread >= 0.0 && min_spread <= 1e300)) return VC_ERR_BAD_ARG;
  int rc = fetch_sums(d);
  if (rc != VC_OK) return rc;
  d->have_fit = d->fit_from_sums = false;
  std::vector<double> a(d->ncells), b(d->ncells);
  std::vector<int> status(d->ncells);
  double c[3], rms[3];
  if (!vc::dc_fit(d->sums.data(), d->ncells, degree, (double)min_count, min_spread, c, a.data(), b.data(), status.data(), rms)) return VC_ERR_NUMERIC;
  d->a = a; d->b = b; d->status = status;
  std::memcpy(d->poly.c, c, 24); std::memcpy(d->rms, rms, 24);
  d->degree = degree;
  rc = upload_fit(d);
  if (rc != VC_OK) return rc;
  d->have_fit = d->fit_from_sums = true;
  return VC_OK;
}
int vc_depthcal_get_fit(vc_depthcal* d, double c[3], double* a, double* b, int* status, double rms[3], int* degree) {
  if (!d || !d->have_fit) return VC_ERR_BAD_ARG;
  if (c) std::memcpy(c, d->poly.c, 24);
  if (a) std::memcpy(a, d->a.data(), d->ncells * sizeof(double));
  if (b) std::memcpy(b, d->b.data(), d->ncells * sizeof(double));
  if (status) std::memcpy(status, d->status.data(), d->ncells * sizeof(int));
  if (rms) std::memcpy(rms, d->rms, 24);
  if (degree) *degree = d->degree;
  return VC_OK;
}
int vc_depthcal_set_fit(vc_depthcal* d, int degree, const double c[3], const double* a, const double* b) {
  if (!d || degree < 0 || degree > 2 || !c || !a || !b) return VC_ERR_BAD_ARG;
  for (int k = 0; k < 3; ++k) if (!std::isfinite(c[k])) return VC_ERR_BAD_ARG;
  for (int k = 0; k < d->ncells; ++k) if (!std::isfinite(a[k]) || !std::isfinite(b[k])) return VC_ERR_BAD_ARG;
  d->have_fit = d->fit_from_sums = false;
  std::memcpy(d->poly.c, c, 24);
  d->a.assign(a, a + d->ncells); d->b.assign(b, b + d->ncells);
  for (int k = 0; k < d->ncells; ++k) d->status[k] = b[k] != 0.0 ? vc::kDcFitted : a[k] != 0.0 ? vc::kDcOffsetOnly : vc::kDcTooFew;      // (what the numbers say)
  const double nan = std::nan("");
  d->rms[0] = d->rms[1] = d->rms[2] = nan;                         // (a fit that was set has no residuals)
  d->degree = degree;
  const int rc = upload_fit(d);
  if (rc != VC_OK) return rc;
  d->have_fit = true;
  return VC_OK;
}

int vc_depthcal_apply(vc_depthcal* d, int n, const unsigned short* src, int src_pitch, long long src_stride, unsigned short* dst, int dst_pitch, long long dst_stride,
                      int interp, long long* counters) {
  if (!d || n < 0 || n > kMaxImages || (interp != vc::kDcInterpCell && interp != vc::kDcInterpBilinear) || !d->have_fit) return VC_ERR_BAD_ARG;
  if (n == 0) return VC_OK;
  if (!images_ok(n, src, src_pitch, src_stride, d->p.w, d->p.h) || !images_ok(n, dst, dst_pitch, dst_stride, d->p.w, d->p.h)) return VC_ERR_BAD_ARG;
  DcBatch dev, host;
  const int rc = begin_call(d, n, kCallApply, &dev, &host);
  if (rc != VC_OK) return rc;
  pack_images(d, host.depth, reinterpret_cast<const unsigned char*>(src), n, src_pitch, src_stride);
  if (hipMemcpyAsync(dev.depth, host.depth, d->img_stride() * n, hipMemcpyHostToDevice, d->stream) != hipSuccess) return VC_ERR_NO_DEVICE;
  launch_apply(d, n, d->poly, d->d_a, d->d_b, interp, DcImages{dev.depth, d->img_stride()}, DcImages{dev.out_depth, d->img_stride()}, dev.counters);
  // one download: [counters | depth]
  const size_t down = (size_t)(dev.out_depth - reinterpret_cast<unsigned char*>(dev.counters)) + d->img_stride() * n;
  if (hipGetLastError() != hipSuccess || hipMemcpyAsync(host.counters, dev.counters, down, hipMemcpyDeviceToHost, d->stream) != hipSuccess ||
      hipStreamSynchronize(d->stream) != hipSuccess) return VC_ERR_NO_DEVICE;
  d->in_flight = false;
  const size_t row = 2 * (size_t)d->p.w;                           // only the pixels: a row's padding is the caller's
  for (int k = 0; k < n; ++k)
    for (int y = 0; y < d->p.h; ++y)
      std::memcpy(reinterpret_cast<unsigned char*>(dst) + (size_t)k * dst_stride + (size_t)y * dst_pitch, host.out_depth + (size_t)k * d->img_stride() + y * row, row);
  if (counters) std::memcpy(counters, host.counters, (size_t)3 * n * 8);
  return VC_OK;
}

int vc_time_depthcal(vc_depthcal* d, int n_images, int reps, double out_ms[3]) {
  if (!d || n_images < 1 || n_images > kMaxImages || reps < 1 || !out_ms) return VC_ERR_BAD_ARG;
  if (hipSetDevice(d->device) != hipSuccess) return VC_ERR_NO_DEVICE;
  if (d->in_flight) (void)hipStreamSynchronize(d->stream);
  // staging of its own shape: [frames | depth] up; partial, counters, sums and a correction of zeros, out_depth on the device only
  const int n = n_images;
  DcFrame* frames[2]; unsigned char* depth[2]; double* partial = nullptr; u64* counters = nullptr; double* running = nullptr; double* ab = nullptr;
  unsigned char* out_depth = nullptr;
  auto carve = [&](int side, vch::Carver q) {
    frames[side] = q.take<DcFrame>(n); depth[side] = q.take<unsigned char>(d->img_stride() * n);
    if (side == 0) {
      partial = q.take<double>((size_t)n * d->nchunks * vc::kDcSums); counters = q.take<u64>((size_t)vc::kDcCounters * n);
      running = q.take<double>((size_t)d->ncells * vc::kDcSums); ab = q.take<double>(d->ncells);
      out_depth = q.take<unsigned char>(d->img_stride() * n);
    }
    return q.bytes();
  };
  if (!reserve(d, carve(0, vch::Carver()), carve(1, vch::Carver()))) return VC_ERR_NO_DEVICE;
  carve(0, vch::Carver(d->d_buf)); carve(1, vch::Carver(d->h_buf));
  d->in_flight = true;
  // device-resident inputs: the camera v_ref counts above the middle of the board and looking straight at it, a surface of v_ref +- 16
  const double height = d->p.v_ref * d->p.unit;
  for (int k = 0; k < n; ++k) {
    DcFrame& f = frames[1][k];
    const double R[9] = {1, 0, 0, 0, -1, 0, 0, 0, -1};
    std::memcpy(f.R, R, sizeof(R));
    f.c[0] = 0.5 * (d->p.rect[0] + d->p.rect[2]); f.c[1] = 0.5 * (d->p.rect[1] + d->p.rect[3]); f.c[2] = height * (1.0 + 0.01 * k);
    unsigned short* img = reinterpret_cast<unsigned short*>(depth[1] + (size_t)k * d->img_stride());
    const int base = (int)fmin(fmax(d->p.v_ref, 17.0), 65500.0);
    for (size_t e = 0; e < d->npix(); ++e) img[e] = (unsigned short)(base - 16 + (int)((3 * e + 11 * k) % 33));
  }
  const size_t up = (size_t)(depth[0] - reinterpret_cast<unsigned char*>(frames[0])) + d->img_stride() * n;
  if (hipMemcpyAsync(frames[0], frames[1], up, hipMemcpyHostToDevice, d->stream) != hipSuccess ||
      hipMemsetAsync(running, 0, (size_t)d->ncells * vc::kDcSums * sizeof(double), d->stream) != hipSuccess ||
      hipMemsetAsync(ab, 0, d->ncells * sizeof(double), d->stream) != hipSuccess) return VC_ERR_NO_DEVICE;
  const DcImages src{depth[0], d->img_stride()};
  DcPoly poly = d->poly;
  poly.c[0] = 1.0; poly.c[1] = poly.c[2] = 0.0;
  for (int what = 0; what < 3; ++what) {
    auto launch = [&]() {                              // (the table a launch rewrites is the same table; the sums of the timer are its own)
      if (what == 0) launch_rays(d);
      else if (what == 1) launch_add(d, n, src, frames[0], partial, counters, running);
      else launch_apply(d, n, poly, ab, ab, vc::kDcInterpBilinear, src, DcImages{out_depth, d->img_stride()}, counters);
    };
    const int rc = vch::time_back_to_back(d->stream, reps, launch, &out_ms[what]);
    if (rc != VC_OK) return rc;
  }
  d->in_flight = false;
  return VC_OK;
}

}  // extern "C"
