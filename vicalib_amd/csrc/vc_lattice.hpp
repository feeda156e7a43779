// vc_lattice.hpp -- the one lattice-sweep core under the comparer (vc_compare.hip), the converter (vc_convert.hip), the uncertainty map
// (vc_uncertainty.hip) and the stereo uncertainty map (vc_stereo_uncertainty.hip, which folds one record per depth plane and launches
// k_lat_reduce itself); included by those four files only.  All of them put a gx * gy lattice over a camera (CmpPlan, cmp_sample,
// vc_compare.hpp), sweep it with 256-thread workgroups that leave one partial record per workgroup, fold the partials with a one-wavefront
// kernel and fetch the folded record with one synchronisation.  What that takes is here once:
//   lat_block_record  a workgroup's record: sums by wave_allsum, the four waves in wave order; optionally the largest value with its sample
//   lat_ring_walk     the rings of a workgroup: thread k owns ring k and walks the 256 entries in thread order
//   k_lat_reduce      one wavefront: lane c folds column c of the workgroup records in workgroup order
//   LatticeHandle     device, stream, the one device allocation, the pinned record, and the one synchronisation of a sweep
// The bits of every result of the three tools depend on the order of these sums and on how the maxima break ties: change either here and
// all three change together.  Nothing below multiplies: additions, comparisons and moves only, so there is nothing for the compiler to
// contract into a fused multiply-add.  The per-sample arithmetic is in vc_compare.hpp, vc_convert.hpp and vc_uncertainty.hpp.
#pragma once
#include <hip/hip_runtime.h>
#include "vc_kutil.hpp"
#include "vc_hostutil.hpp"
#include "vc_compare.hpp"

namespace vc {

constexpr int kLatNone = -1;                   // k_lat_reduce: no carried maximum, no ring columns
constexpr int kLatRingDoubles = 4;             // a ring's record: count, invalid, a sum, a maximum

// The record of a workgroup of four waves from per-lane values: columns 0 .. N - 1 are the sums of x[k] (wave_allsum, then the four waves as
// ((w0 + w1) + w2) + w3); thread c writes column c.  With ARGMAX, columns N and N + 1 are the largest `best` and its sample `best_i`, the
// lowest sample of equal ones (wave_argmax_low; a lane without an entry brings -1.0 and -1).  N is a compile-time constant: x stays in
// registers.  Reached by every thread of the workgroup: there is a __syncthreads() inside, and it is the barrier that orders a caller's LDS
// entries before lat_ring_walk.
template <int N, bool ARGMAX = false>
__device__ __forceinline__ void lat_block_record(double* rec, const double (&x)[N], double best = -1.0, int best_i = -1) {
  __shared__ double s_w[4][N + (ARGMAX ? 2 : 0)];
  const int wave = threadIdx.x >> 6, t = threadIdx.x;
  const bool first = (threadIdx.x & 63) == 0;
#pragma unroll
  for (int k = 0; k < N; ++k) {
    const double sum = wave_allsum(x[k]);
    if (first) s_w[wave][k] = sum;
  }
  if (ARGMAX) {
    wave_argmax_low(&best, &best_i);
    if (first) { s_w[wave][N] = best; s_w[wave][N + 1] = (double)best_i; }
  }
  __syncthreads();
  if (t < N) rec[t] = ((s_w[0][t] + s_w[1][t]) + s_w[2][t]) + s_w[3][t];
  if (ARGMAX && t == N) {                                          // waves hold ascending samples: a later wave wins only when larger
    double b = s_w[0][N], bi = s_w[0][N + 1];
#pragma unroll
    for (int w = 1; w < 4; ++w) if (s_w[w][N] > b) { b = s_w[w][N]; bi = s_w[w][N + 1]; }
    rec[N] = b; rec[N + 1] = bi;
  }
}

// The rings of a workgroup from its 256 LDS entries: s_ring[j] the ring of thread j's sample (-1: none), s_key[j] the value whose maximum
// is kept (negative: the sample is invalid), s_val[j] the value that is summed (s_key itself where they are the same).  Thread k < n_rings
// owns ring k and walks the entries in thread order: rings[4 k ..] = count, invalid, sum, maximum (-1.0: none).  The entries must have been
// written before a barrier of the whole workgroup: lat_block_record's.
__device__ __forceinline__ void lat_ring_walk(double* rings, int n_rings, const int* s_ring, const double* s_val, const double* s_key) {
  if ((int)threadIdx.x >= n_rings) return;
  double rc = 0.0, ri = 0.0, rs = 0.0, rm = -1.0;
  for (int j = 0; j < 256; ++j) {
    if (s_ring[j] != (int)threadIdx.x) continue;
    const double q = s_key[j];
    if (q >= 0.0) { rc += 1.0; rs += s_val[j]; rm = q > rm ? q : rm; } else ri += 1.0;
  }
  double* r = rings + kLatRingDoubles * threadIdx.x;
  r[0] = rc; r[1] = ri; r[2] = rs; r[3] = rm;
}

}  // namespace vc

namespace {

// Columns 0 .. m - 1 of n_wg records of `stride` doubles folded in workgroup order: a plain column is added up from 0.0.  With MAXIMA, column
// `worst` (or kLatNone) is a maximum that carries column worst + 1, its sample; from column `ring0` (or kLatNone) on, every fourth column is a
// maximum.  Maxima start from -1.0 and strictly larger wins: workgroups hold ascending samples, so the first of equal ones stays.
// With MAXIMA every lane walks the records once and keeps both the sum and the maximum of its column -- the kinds of column differ in what is
// stored, not in a loop of their own, which the one wavefront would run one after the other, each at a memory round trip per record.  A record
// of plain sums (MAXIMA = false) keeps the bare loop: the second instantiation is there because the merged loop measured 6 - 24 % slower on it.
// (Internal linkage: each of the three translation units has its own copy of the one definition.)
template <bool MAXIMA>
__global__ __launch_bounds__(64) void k_lat_reduce(const double* __restrict__ part, int n_wg, int stride, int m, int worst, int ring0, double* __restrict__ out) {
  for (int c = threadIdx.x; c < m; c += 64) {
    const bool is_worst = MAXIMA && c == worst, is_max = is_worst || (MAXIMA && ring0 >= 0 && c >= ring0 && ((c - ring0) & 3) == 3);
    if (MAXIMA && worst >= 0 && c == worst + 1) continue;          // (written with column `worst`)
    double t = 0.0, b = -1.0, bi = -1.0;
    for (int g = 0; g < n_wg; ++g) {
      const double* p = part + (size_t)g * stride + c;
      const double x = p[0], xi = is_worst ? p[1] : -1.0;
      t += x;
      if (MAXIMA && x > b) { b = x; bi = xi; }
    }
    out[c] = is_max ? b : t;
    if (is_worst) out[c + 1] = bi;
  }
}

}  // namespace

namespace vc {

// What a lattice tool's handle derives from: its device, its stream, ONE device allocation -- the tool's arrays (device_bytes, sized and
// handed out by the tool's Carver sequence) with the folded record d_res behind them -- and the pinned host copy of that record.
struct LatticeHandle {
  int device = 0;
  hipStream_t stream = nullptr;
  unsigned char* d_buf = nullptr;
  double* d_res = nullptr;             // the folded record of the sweep in flight (k_lat_reduce's out)
  double* h_res = nullptr;             // pinned: its host copy
  bool in_flight = false;

  // false: no such device or an allocation failed; whatever was got is freed again
  bool open(int dev, size_t device_bytes, int result_doubles) {
    if (vch::open_device(dev) != VC_OK) return false;
    device = dev;
    if (hipStreamCreate(&stream) != hipSuccess || hipMalloc((void**)&d_buf, device_bytes + (size_t)result_doubles * 8) != hipSuccess ||
        hipHostMalloc((void**)&h_res, (size_t)result_doubles * 8, hipHostMallocDefault) != hipSuccess) { close(); return false; }
    d_res = reinterpret_cast<double*>(d_buf + device_bytes);       // (a Carver's bytes() is a multiple of 256)
    return true;
  }
  void close() {
    (void)hipSetDevice(device);
    if (stream) { (void)hipStreamSynchronize(stream); (void)hipStreamDestroy(stream); }
    (void)hipFree(d_buf);
    if (h_res) (void)hipHostFree(h_res);
    stream = nullptr; d_buf = nullptr; d_res = nullptr; h_res = nullptr;
  }
  // before a call launches: the handle's device current, and the stream drained if an earlier call left through an error path
  bool settle() {
    if (hipSetDevice(device) != hipSuccess) return false;
    if (in_flight) { (void)hipStreamSynchronize(stream); in_flight = false; }
    return true;
  }
  // the first m doubles of the folded record of what was just enqueued, in h_res: the one synchronisation of a sweep (m = 0: none to fetch)
  bool fetch(int m) {
    in_flight = true;
    if (hipGetLastError() != hipSuccess || (m > 0 && hipMemcpyAsync(h_res, d_res, (size_t)m * 8, hipMemcpyDeviceToHost, stream) != hipSuccess) ||
        hipStreamSynchronize(stream) != hipSuccess) return false;
    in_flight = false;
    return true;
  }
  void reduce(const double* part, int n_wg, int stride, int m, int worst = kLatNone, int ring0 = kLatNone) {
    if (worst == kLatNone && ring0 == kLatNone) hipLaunchKernelGGL(k_lat_reduce<false>, dim3(1), dim3(64), 0, stream, part, n_wg, stride, m, worst, ring0, d_res);
    else hipLaunchKernelGGL(k_lat_reduce<true>, dim3(1), dim3(64), 0, stream, part, n_wg, stride, m, worst, ring0, d_res);
  }
};

}  // namespace vc
