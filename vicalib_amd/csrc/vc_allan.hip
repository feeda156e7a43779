// vc_allan.hip -- the noise of an IMU from a static log (gfx950, wave64, fp64 throughout): the handle vc_allan.  vc_allan.hpp has the arithmetic.
//
// The log lives on the device channel-major: y[c][0 .. n-1] and the prefix sums S[c][0 .. n] (n + 1 doubles per channel), so lanes run along
// the sample index and every access is coalesced.
//  k_allan_totals       grid (blocks of 256 samples, channel): the block's sum of y (pass 0) or of y - mean (pass 1).
//  k_allan_mean         one workgroup per channel: the block totals of pass 0 added tile by tile (256 totals each) in block order -> the mean.
//  k_allan_scan_totals  one workgroup per channel: the exclusive scan of the block totals of pass 1, tile by tile with a running carry.
//  k_allan_scan         grid as k_allan_totals: the inclusive scan of y - mean inside the block plus the block's carry -> S[c][i + 1].
//  k_allan_sweep        grid (chunk of kAllanChunk terms, factor, channel): the lanes stride the chunk, lane partials go through wave_allsum,
//                       the four waves are added in wave order through LDS, one partial per (factor, channel, chunk).
//  k_allan_finish       one thread per (factor, channel): the chunk partials added in chunk order, divided by 2 m^2 terms.
//  k_allan_quiet        one thread per window start: one byte, 1 = quiet.
// Separate launches order the steps: no workgroup waits on another inside a launch, no flag, no spin.  No floating-point atomic: the order
// of every sum is fixed by n, the range, the factor and the constants of vc_allan.hpp, so two runs give the same bits and a channel's bits
// do not depend on the other five.  No CPU fallback: without a device vc_allan_create fails.
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstring>
#include <vector>
#include "../../include/vicalib_amd.h"
#include "vc_kutil.hpp"
#include "vc_hostutil.hpp"
#include "vc_allan.hpp"

namespace {

constexpr int kB = vc::kAllanScanBlock;
static_assert(kB == 256, "the scan kernels run one sample per thread of a 256-thread workgroup");

// the sum of the workgroup's values in every thread: the xor butterfly inside a wave, then the four waves in wave order
__device__ __forceinline__ double block_sum(double v, double* lds /* 4 */) {
  const int wave = threadIdx.x >> 6;
  v = vc::wave_allsum(v);
  __syncthreads();                                   // (the previous use of lds is over)
  if ((threadIdx.x & 63) == 0) lds[wave] = v;
  __syncthreads();
  return ((lds[0] + lds[1]) + lds[2]) + lds[3];
}
// the inclusive (EXCL = false) or exclusive scan of the workgroup's values in thread order, and their total
template <bool EXCL>
__device__ __forceinline__ double block_scan(double v, double* lds /* 4 */, double* total) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  double s = v;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const double t = __shfl_up(s, o, 64);
    if (lane >= o) s += t;
  }
  __syncthreads();
  if (lane == 63) lds[wave] = s;
  __syncthreads();
  double off = 0.0;
  if (wave > 0) off = lds[0];
  if (wave > 1) off += lds[1];
  if (wave > 2) off += lds[2];
  *total = ((lds[0] + lds[1]) + lds[2]) + lds[3];
  if (EXCL) {
    double e = __shfl_up(s, 1, 64);
    if (lane == 0) e = 0.0;
    return off + e;
  }
  return off + s;
}

__global__ __launch_bounds__(256) void k_allan_totals(const double* __restrict__ y, int n, int n_blocks, const double* __restrict__ mean /* null: pass 0 */,
                                                      double* __restrict__ tot) {
  __shared__ double lds[4];
  const int c = blockIdx.y, i = blockIdx.x * kB + threadIdx.x;
  const double mu = mean ? mean[c] : 0.0;
  const double v = i < n ? y[(size_t)c * n + i] - mu : 0.0;
  const double s = block_sum(v, lds);
  if (threadIdx.x == 0) tot[(size_t)c * n_blocks + blockIdx.x] = s;
}

__global__ __launch_bounds__(256) void k_allan_mean(const double* __restrict__ tot, int n, int n_blocks, double* __restrict__ mean) {
  __shared__ double lds[4];
  const int c = blockIdx.x;
  double carry = 0.0;
  for (int t0 = 0; t0 < n_blocks; t0 += kB) {
    const int b = t0 + threadIdx.x;
    carry += block_sum(b < n_blocks ? tot[(size_t)c * n_blocks + b] : 0.0, lds);
  }
  if (threadIdx.x == 0) mean[c] = carry / (double)n;
}

__global__ __launch_bounds__(256) void k_allan_scan_totals(const double* __restrict__ tot, int n_blocks, double* __restrict__ carry_in) {
  __shared__ double lds[4];
  const int c = blockIdx.x;
  double carry = 0.0;
  for (int t0 = 0; t0 < n_blocks; t0 += kB) {
    const int b = t0 + threadIdx.x;
    double total;
    const double e = block_scan<true>(b < n_blocks ? tot[(size_t)c * n_blocks + b] : 0.0, lds, &total);
    if (b < n_blocks) carry_in[(size_t)c * n_blocks + b] = carry + e;
    carry += total;
  }
}

__global__ __launch_bounds__(256) void k_allan_scan(const double* __restrict__ y, int n, int n_blocks, const double* __restrict__ mean,
                                                    const double* __restrict__ carry_in, double* __restrict__ S) {
  __shared__ double lds[4];
  const int c = blockIdx.y, i = blockIdx.x * kB + threadIdx.x;
  const double v = i < n ? y[(size_t)c * n + i] - mean[c] : 0.0;
  double total;
  const double s = block_scan<false>(v, lds, &total);
  double* Sc = S + (size_t)c * ((size_t)n + 1);
  if (i < n) Sc[i + 1] = carry_in[(size_t)c * n_blocks + blockIdx.x] + s;      // i + 1 <= n: the channel's last entry
  if (i == 0) Sc[0] = 0.0;
}

// samples [first, first + count) of every channel; factor j = blockIdx.y; the partial of chunk blockIdx.x
__global__ __launch_bounds__(256) void k_allan_sweep(const double* __restrict__ S, int n, int first, int count, const int* __restrict__ m_list, int n_m,
                                                     int max_chunks, double* __restrict__ part) {
  __shared__ double lds[4];
  const int j = blockIdx.y, c = blockIdx.z;
  const int m = m_list[j];
  const int terms = vc::allan_terms(count, m);
  const int k0 = blockIdx.x * vc::kAllanChunk;
  if (k0 >= terms) return;                                           // (the whole workgroup: this factor has fewer chunks)
  const int k_end = min(k0 + vc::kAllanChunk, terms);
  const double* Sc = S + (size_t)c * ((size_t)n + 1) + first;        // the largest index read is terms - 1 + 2m = count: first + count <= n
  double acc = 0.0;
  for (int k = k0 + (int)threadIdx.x; k < k_end; k += 256) acc += vc::allan_term(Sc, k, m);
  const double s = block_sum(acc, lds);
  if (threadIdx.x == 0) part[((size_t)c * n_m + j) * max_chunks + blockIdx.x] = s;
}

__global__ __launch_bounds__(256) void k_allan_finish(const double* __restrict__ part, int count, const int* __restrict__ m_list, int n_m, int max_chunks,
                                                      double* __restrict__ avar /* 6 x n_m */) {
  const int t = blockIdx.x * 256 + threadIdx.x;
  if (t >= vc::kAllanChannels * n_m) return;
  const int j = t % n_m;
  const int m = m_list[j], terms = vc::allan_terms(count, m), chunks = vc::allan_chunks(terms);      // chunks <= max_chunks: terms <= count - 1
  const double* p = part + (size_t)t * max_chunks;
  double s = 0.0;
  for (int q = 0; q < chunks; ++q) s += p[q];
  avar[t] = vc::allan_avar(s, m, terms);
}

__global__ __launch_bounds__(256) void k_allan_quiet(const double* __restrict__ S, int n, int W, int n_starts, double gyro_thr, double accel_thr,
                                                     unsigned char* __restrict__ mask) {
  const int k = blockIdx.x * 256 + threadIdx.x;                      // k + 2W <= n_starts - 1 + 2W = n
  if (k < n_starts) mask[k] = vc::allan_quiet(S, (size_t)n + 1, k, W, gyro_thr, accel_thr) ? 1 : 0;
}

}  // namespace

struct vc_allan {
  int device = 0, n = 0, n_blocks = 0, first = 0, count = 0;
  double tau0 = 0.0, dt_min = 0.0, dt_max = 0.0, mean[6] = {0, 0, 0, 0, 0, 0};
  long long irregular = 0;
  hipStream_t stream = nullptr;
  unsigned char* buf = nullptr;                    // y, S, totals, carries, means, the quiet mask: one allocation
  double *y = nullptr, *S = nullptr, *tot = nullptr, *carry = nullptr, *d_mean = nullptr;
  unsigned char* mask = nullptr;
  unsigned char* run_buf = nullptr;                // factors, partials and results of a run: grows with n_m
  size_t run_bytes = 0;
};

namespace {

void launch_scan(vc_allan* h) {
  const dim3 grid(h->n_blocks, vc::kAllanChannels);
  hipLaunchKernelGGL(k_allan_totals, grid, dim3(256), 0, h->stream, h->y, h->n, h->n_blocks, (const double*)nullptr, h->tot);
  hipLaunchKernelGGL(k_allan_mean, dim3(vc::kAllanChannels), dim3(256), 0, h->stream, h->tot, h->n, h->n_blocks, h->d_mean);
  hipLaunchKernelGGL(k_allan_totals, grid, dim3(256), 0, h->stream, h->y, h->n, h->n_blocks, (const double*)h->d_mean, h->tot);
  hipLaunchKernelGGL(k_allan_scan_totals, dim3(vc::kAllanChannels), dim3(256), 0, h->stream, h->tot, h->n_blocks, h->carry);
  hipLaunchKernelGGL(k_allan_scan, grid, dim3(256), 0, h->stream, h->y, h->n, h->n_blocks, h->d_mean, h->carry, h->S);
}

struct RunArrays { int* m; double* part; double* avar; int max_chunks; };
size_t carve_run(vch::Carver q, int n_m, int max_chunks, RunArrays* a) {
  a->m = q.take<int>((size_t)n_m);
  a->part = q.take<double>((size_t)vc::kAllanChannels * n_m * max_chunks);
  a->avar = q.take<double>((size_t)vc::kAllanChannels * n_m);
  a->max_chunks = max_chunks;
  return q.bytes();
}
void launch_sweep(vc_allan* h, const RunArrays& a, int n_m) {
  hipLaunchKernelGGL(k_allan_sweep, dim3(a.max_chunks, n_m, vc::kAllanChannels), dim3(256), 0, h->stream, h->S, h->n, h->first, h->count, a.m, n_m,
                     a.max_chunks, a.part);
  hipLaunchKernelGGL(k_allan_finish, dim3((vc::kAllanChannels * n_m + 255) / 256), dim3(256), 0, h->stream, a.part, h->count, a.m, n_m, a.max_chunks, a.avar);
}
bool factors_ok(const vc_allan* h, int n_m, const int* m) {
  if (n_m < 1 || n_m > vc::kAllanMaxFactors || !m) return false;
  for (int j = 0; j < n_m; ++j)
    if (m[j] < 1 || m[j] > h->count / 2) return false;
  return true;
}
// the factors on the device and room for the partials of the current range
int prepare_run(vc_allan* h, int n_m, const int* m, RunArrays* a) {
  if (hipSetDevice(h->device) != hipSuccess) return VC_ERR_NO_DEVICE;
  int m_min = m[0];
  for (int j = 1; j < n_m; ++j) m_min = m[j] < m_min ? m[j] : m_min;
  const int max_chunks = vc::allan_chunks(vc::allan_terms(h->count, m_min));
  const size_t need = carve_run(vch::Carver(), n_m, max_chunks, a);
  if (need > h->run_bytes) {
    if (h->run_buf) (void)hipFree(h->run_buf);
    h->run_buf = nullptr; h->run_bytes = 0;
    if (hipMalloc((void**)&h->run_buf, need) != hipSuccess) return VC_ERR_NO_DEVICE;
    h->run_bytes = need;
  }
  carve_run(vch::Carver(h->run_buf), n_m, max_chunks, a);
  if (hipMemcpyAsync(a->m, m, (size_t)n_m * sizeof(int), hipMemcpyHostToDevice, h->stream) != hipSuccess) return VC_ERR_NO_DEVICE;
  return VC_OK;
}

}  // namespace

extern "C" int vc_allan_create(int device, int n, const double* gyro, const double* accel, const double* time, vc_allan** out) {
  if (out) *out = nullptr;
  if (!out || !gyro || !accel || !time || n < 2) return VC_ERR_BAD_ARG;
  if (n > vc::kAllanMaxN) return VC_ERR_UNSUPPORTED;               // (before anything is read)
  const size_t N = (size_t)n;
  if (!std::isfinite(time[0])) return VC_ERR_BAD_ARG;
  for (size_t i = 1; i < N; ++i)
    if (!std::isfinite(time[i]) || !(time[i] > time[i - 1])) return VC_ERR_BAD_ARG;
  std::vector<double> y(6 * N);                                   // channel-major
  for (size_t i = 0; i < N; ++i)
    for (int c = 0; c < 3; ++c) {
      const double g = gyro[3 * i + c], a = accel[3 * i + c];
      if (!std::isfinite(g) || !std::isfinite(a)) return VC_ERR_BAD_ARG;
      y[(size_t)c * N + i] = g; y[(size_t)(3 + c) * N + i] = a;
    }
  if (vch::open_device(device) != VC_OK) return VC_ERR_NO_DEVICE;
  vc_allan* h = new vc_allan;
  h->device = device; h->n = n; h->n_blocks = (n + kB - 1) / kB; h->first = 0; h->count = n;
  h->tau0 = (time[N - 1] - time[0]) / (double)(n - 1);
  h->dt_min = h->dt_max = time[1] - time[0];
  for (size_t i = 1; i < N; ++i) {
    const double dt = time[i] - time[i - 1];
    h->dt_min = dt < h->dt_min ? dt : h->dt_min; h->dt_max = dt > h->dt_max ? dt : h->dt_max;
    if (!(dt >= 0.5 * h->tau0 && dt <= 1.5 * h->tau0)) ++h->irregular;
  }
  auto carve = [&](vch::Carver q) {
    h->y = q.take<double>(6 * N); h->S = q.take<double>(6 * (N + 1)); h->tot = q.take<double>(6 * (size_t)h->n_blocks);
    h->carry = q.take<double>(6 * (size_t)h->n_blocks); h->d_mean = q.take<double>(6); h->mask = q.take<unsigned char>(N);
    return q.bytes();
  };
  bool ok = hipStreamCreate(&h->stream) == hipSuccess && hipMalloc((void**)&h->buf, carve(vch::Carver())) == hipSuccess;
  if (ok) {
    carve(vch::Carver(h->buf));
    ok = hipMemcpyAsync(h->y, y.data(), 6 * N * sizeof(double), hipMemcpyHostToDevice, h->stream) == hipSuccess;
  }
  if (ok) {
    launch_scan(h);
    ok = hipGetLastError() == hipSuccess && hipMemcpyAsync(h->mean, h->d_mean, 6 * sizeof(double), hipMemcpyDeviceToHost, h->stream) == hipSuccess;
  }
  ok = ok && hipStreamSynchronize(h->stream) == hipSuccess;
  if (!ok) { vc_allan_destroy(h); return VC_ERR_NO_DEVICE; }
  *out = h;
  return VC_OK;
}

extern "C" void vc_allan_destroy(vc_allan* h) {
  if (!h) return;
  (void)hipSetDevice(h->device);
  if (h->stream) (void)hipStreamSynchronize(h->stream);
  if (h->run_buf) (void)hipFree(h->run_buf);
  if (h->buf) (void)hipFree(h->buf);
  if (h->stream) (void)hipStreamDestroy(h->stream);
  delete h;
}

extern "C" int vc_allan_get(vc_allan* h, int* n, double* tau0, double* dt_min, double* dt_max, double means[6], long long* irregular, int range[2]) {
  if (!h) return VC_ERR_BAD_ARG;
  if (n) *n = h->n;
  if (tau0) *tau0 = h->tau0;
  if (dt_min) *dt_min = h->dt_min;
  if (dt_max) *dt_max = h->dt_max;
  if (means) std::memcpy(means, h->mean, sizeof(h->mean));
  if (irregular) *irregular = h->irregular;
  if (range) { range[0] = h->first; range[1] = h->count; }
  return VC_OK;
}

extern "C" int vc_allan_set_range(vc_allan* h, int first, int count) {
  if (!h || first < 0 || count < 2 || first > h->n - count) return VC_ERR_BAD_ARG;
  h->first = first; h->count = count;
  return VC_OK;
}

extern "C" int vc_allan_static(vc_allan* h, int window, double gyro_thr, double accel_thr, int range_out[2], int* n_quiet) {
  if (!h || window < 1 || window >= h->n - window || std::isnan(gyro_thr) || std::isnan(accel_thr)) return VC_ERR_BAD_ARG;      // 2 window >= n
  const int n_starts = h->n - 2 * window + 1;
  int k0 = 0, k1 = n_starts - 1, quiet = n_starts;
  if (gyro_thr > 0.0 || accel_thr > 0.0) {                          // (both tests off: every start is quiet, the whole log)
    if (hipSetDevice(h->device) != hipSuccess) return VC_ERR_NO_DEVICE;
    std::vector<unsigned char> mask((size_t)n_starts);
    hipLaunchKernelGGL(k_allan_quiet, dim3((n_starts + 255) / 256), dim3(256), 0, h->stream, h->S, h->n, window, n_starts, gyro_thr, accel_thr, h->mask);
    if (hipGetLastError() != hipSuccess || hipMemcpyAsync(mask.data(), h->mask, (size_t)n_starts, hipMemcpyDeviceToHost, h->stream) != hipSuccess ||
        hipStreamSynchronize(h->stream) != hipSuccess)
      return VC_ERR_NO_DEVICE;
    if (!vc::allan_longest_run(mask.data(), n_starts, &k0, &k1, &quiet)) {
      if (n_quiet) *n_quiet = 0;
      if (range_out) { range_out[0] = h->first; range_out[1] = h->count; }
      return 1;                                                     // no start is quiet: the range stays
    }
  }
  h->first = k0; h->count = k1 + 2 * window - k0;
  if (n_quiet) *n_quiet = quiet;
  if (range_out) { range_out[0] = h->first; range_out[1] = h->count; }
  return VC_OK;
}

extern "C" int vc_allan_run(vc_allan* h, int n_m, const int* m, double* avar, int* terms) {
  if (!h || !avar || !factors_ok(h, n_m, m)) return VC_ERR_BAD_ARG;
  RunArrays a;
  const int rc = prepare_run(h, n_m, m, &a);
  if (rc != VC_OK) return rc;
  launch_sweep(h, a, n_m);
  if (hipGetLastError() != hipSuccess ||
      hipMemcpyAsync(avar, a.avar, (size_t)vc::kAllanChannels * n_m * sizeof(double), hipMemcpyDeviceToHost, h->stream) != hipSuccess ||
      hipStreamSynchronize(h->stream) != hipSuccess)
    return VC_ERR_NO_DEVICE;
  if (terms)
    for (int j = 0; j < n_m; ++j) terms[j] = vc::allan_terms(h->count, m[j]);
  return VC_OK;
}

extern "C" int vc_time_allan(vc_allan* h, int n_m, const int* m, int reps, double out_ms[2]) {
  if (!h || reps < 1 || !out_ms || !factors_ok(h, n_m, m)) return VC_ERR_BAD_ARG;
  RunArrays a;
  int rc = prepare_run(h, n_m, m, &a);
  if (rc != VC_OK) return rc;
  rc = vch::time_back_to_back(h->stream, reps, [&]() { launch_scan(h); }, &out_ms[0]);      // (the same input: the same bits)
  if (rc == VC_OK) rc = vch::time_back_to_back(h->stream, reps, [&]() { launch_sweep(h, a, n_m); }, &out_ms[1]);
  return rc;
}
