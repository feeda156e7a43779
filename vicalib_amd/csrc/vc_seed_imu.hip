// vc_seed_imu.hip -- the inertial seed (gfx950, wave64, fp64 throughout): the rotation camera <- IMU, the time offset, the gyro bias and the
// direction of gravity from the PnP rotations of the frames and the IMU log: vc_seed_imu_sweep, vc_seed_imu.  vc_seed_imu.hpp has the arithmetic.
//
// The log lives on the device channel-major: y[c][0 .. n-1] and the prefix integrals G[c][0 .. n-1], so lanes run along the sample index.
//  k_simu_totals        grid (blocks of 256 samples, channel): the block's sum of the trapezoid increments (sample 0 adds nothing).
//  k_simu_scan_totals   one workgroup per channel: the exclusive scan of the block totals, tile by tile (256 totals each) with a running carry.
//  k_simu_scan          grid as k_simu_totals: the inclusive scan of the increments inside the block plus the block's carry -> G[c][k].
//  k_simu_rates         one thread per interval of two consecutive frames: a_i, 1 / dt, validity.
//  k_simu_sweep         grid (chunk of kSeedImuChunk intervals, lag): the lanes stride the chunk, every interval evaluates G at its two ends
//                       (two bounded bisections in the sample times), the 18 lane moments go through wave_allsum, the four waves are added in
//                       wave order through LDS, one 18-double partial per (lag, chunk).
//  k_simu_finish        one thread per lag: the partials added in chunk order, centred, Horn's rotation, J, the bias, the count.
//  k_simu_gravity       grid (chunk) at one lag and one R_ck: three sums per chunk; the host adds them in chunk order.
// Separate launches order the steps: no workgroup waits on another inside a launch, no flag, no spin.  No floating-point atomic: the order of
// every sum is fixed by the sizes and the constants of vc_seed_imu.hpp, so two runs give the same bits and a lag gives the same bits alone or
// among others.  Every loop's bound is known before the launch.  No CPU fallback: without a device the entry points fail.
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstring>
#include <vector>
#include "../../include/vicalib_amd.h"
#include "vc_kutil.hpp"
#include "vc_hostutil.hpp"
#include "vc_seed_imu.hpp"

namespace {

constexpr int kB = vc::kSeedImuScanBlock;
constexpr int kM = vc::kSeedImuMoments;
static_assert(kB == 256, "the scan kernels run one sample per thread of a 256-thread workgroup");
static_assert(vc::kSeedImuChunk % 256 == 0, "the lanes of a 256-thread workgroup stride a chunk");

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

// the trapezoid between samples k - 1 and k of channel c; nothing for sample 0 and behind the log
__device__ __forceinline__ double increment(const double* __restrict__ t, const double* __restrict__ y, int n, int c, int k) {
  if (k < 1 || k >= n) return 0.0;
  const double* yc = y + (size_t)c * n;
  return vc::simu_prefix_inc(yc[k - 1], yc[k], t[k - 1], t[k]);
}

__global__ __launch_bounds__(256) void k_simu_totals(const double* __restrict__ t, const double* __restrict__ y, int n, int n_blocks, double* __restrict__ tot) {
  __shared__ double lds[4];
  const int c = blockIdx.y, k = blockIdx.x * kB + threadIdx.x;
  const double s = block_sum(increment(t, y, n, c, k), lds);
  if (threadIdx.x == 0) tot[(size_t)c * n_blocks + blockIdx.x] = s;
}

__global__ __launch_bounds__(256) void k_simu_scan_totals(const double* __restrict__ tot, int n_blocks, double* __restrict__ carry_in) {
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

__global__ __launch_bounds__(256) void k_simu_scan(const double* __restrict__ t, const double* __restrict__ y, int n, int n_blocks,
                                                   const double* __restrict__ carry_in, double* __restrict__ G) {
  __shared__ double lds[4];
  const int c = blockIdx.y, k = blockIdx.x * kB + threadIdx.x;
  double total;
  const double s = block_scan<false>(increment(t, y, n, c, k), lds, &total);
  if (k < n) G[(size_t)c * n + k] = carry_in[(size_t)c * n_blocks + blockIdx.x] + s;
}

struct SimuFrames {
  int n_int;                       // intervals: n_frames - 1
  const double* ft;                // n_frames
  const double* fq;                // n_frames x 4
  const unsigned char* ok;         // n_frames
  double* a;                       // n_int x 3
  double* inv_dt;                  // n_int
  unsigned char* valid;            // n_int
  const double* pivot;             // 3
};

__global__ __launch_bounds__(256) void k_simu_rates(SimuFrames f, double max_gap_s) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= f.n_int) return;                                           // (i + 1 <= n_frames - 1)
  double a[3], inv_dt;
  const bool v = vc::simu_cam_rate(f.fq + 4 * (size_t)i, f.fq + 4 * (size_t)(i + 1), f.ok[i] != 0, f.ok[i + 1] != 0, f.ft[i], f.ft[i + 1], max_gap_s, a, &inv_dt);
  f.a[3 * (size_t)i] = a[0]; f.a[3 * (size_t)i + 1] = a[1]; f.a[3 * (size_t)i + 2] = a[2];
  f.inv_dt[i] = inv_dt; f.valid[i] = v ? 1 : 0;
}

// lag lag0 + blockIdx.y, chunk blockIdx.x
__global__ __launch_bounds__(256) void k_simu_sweep(vc::SimuLog L, SimuFrames f, const double* __restrict__ lags, int lag0, int chunks, double* __restrict__ part) {
  __shared__ double lds[4 * kM];
  const int j = lag0 + blockIdx.y;
  const double d = lags[j];
  const int i0 = blockIdx.x * vc::kSeedImuChunk;
  const int i_end = min(i0 + vc::kSeedImuChunk, f.n_int);
  const double p0 = f.pivot[0], p1 = f.pivot[1], p2 = f.pivot[2];
  double m[kM];
#pragma unroll
  for (int q = 0; q < kM; ++q) m[q] = 0.0;
  for (int i = i0 + (int)threadIdx.x; i < i_end; i += 256) {          // at most kSeedImuChunk / 256 rounds
    if (!f.valid[i]) continue;
    double b[3];
    if (!vc::simu_mean3(L, 0, f.ft[i] - d, f.ft[i + 1] - d, f.inv_dt[i], b)) continue;
    const double ar[3] = {f.a[3 * (size_t)i] - p0, f.a[3 * (size_t)i + 1] - p1, f.a[3 * (size_t)i + 2] - p2};
    vc::simu_accumulate(ar, b, m);
  }
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
#pragma unroll
  for (int q = 0; q < kM; ++q) {
    const double s = vc::wave_allsum(m[q]);
    if (lane == 0) lds[wave * kM + q] = s;
  }
  __syncthreads();
  if (threadIdx.x < kM) {
    const int q = threadIdx.x;
    part[((size_t)j * chunks + blockIdx.x) * kM + q] = ((lds[q] + lds[kM + q]) + lds[2 * kM + q]) + lds[3 * kM + q];
  }
}

struct SimuOut { double* J; double* R; double* bias; int* count; double* mom; };

__global__ __launch_bounds__(256) void k_simu_finish(const double* __restrict__ part, int n_lags, int chunks, const double* __restrict__ pivot, int min_valid, SimuOut o) {
  const int j = blockIdx.x * 256 + threadIdx.x;
  if (j >= n_lags) return;
  double m[kM];
#pragma unroll
  for (int q = 0; q < kM; ++q) m[q] = 0.0;
  const double* p = part + (size_t)j * chunks * kM;
  for (int c = 0; c < chunks; ++c)
#pragma unroll
    for (int q = 0; q < kM; ++q) m[q] += p[(size_t)c * kM + q];
  double J, R[9], bias[3];
  int count;
  const double piv[3] = {pivot[0], pivot[1], pivot[2]};
  vc::simu_fit(m, piv, min_valid, &J, R, bias, &count);
  o.J[j] = J; o.count[j] = count;
#pragma unroll
  for (int k = 0; k < 9; ++k) o.R[(size_t)j * 9 + k] = R[k];
#pragma unroll
  for (int k = 0; k < 3; ++k) o.bias[(size_t)j * 3 + k] = bias[k];
#pragma unroll
  for (int q = 0; q < kM; ++q) o.mom[(size_t)j * kM + q] = m[q];
}

struct SimuRot { double r[9]; };

__global__ __launch_bounds__(256) void k_simu_gravity(vc::SimuLog L, SimuFrames f, double d, SimuRot R_ck, double* __restrict__ part /* chunks x 3 */) {
  __shared__ double lds[4 * 3];
  const int i0 = blockIdx.x * vc::kSeedImuChunk;
  const int i_end = min(i0 + vc::kSeedImuChunk, f.n_int);
  double s0 = 0.0, s1 = 0.0, s2 = 0.0;
  for (int i = i0 + (int)threadIdx.x; i < i_end; i += 256) {
    if (!f.valid[i]) continue;
    double abar[3], g[3];
    if (!vc::simu_mean3(L, 3, f.ft[i] - d, f.ft[i + 1] - d, f.inv_dt[i], abar)) continue;
    vc::simu_gravity_term(f.fq + 4 * (size_t)i, R_ck.r, abar, g);
    s0 += g[0]; s1 += g[1]; s2 += g[2];
  }
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  s0 = vc::wave_allsum(s0); s1 = vc::wave_allsum(s1); s2 = vc::wave_allsum(s2);
  if (lane == 0) { lds[wave * 3] = s0; lds[wave * 3 + 1] = s1; lds[wave * 3 + 2] = s2; }
  __syncthreads();
  if (threadIdx.x < 3) {
    const int q = threadIdx.x;
    part[(size_t)blockIdx.x * 3 + q] = ((lds[q] + lds[3 + q]) + lds[6 + q]) + lds[9 + q];
  }
}

// The data of one call on the device: the log with its prefix integrals, the frames with their rates.  Not a handle of the C ABI: it lives
// for one entry point.
struct SimuDevice {
  int n = 0, n_blocks = 0, n_frames = 0, n_int = 0, chunks = 0, min_valid = 3;
  double max_gap_s = 0.0;
  hipStream_t stream = nullptr;
  unsigned char* buf = nullptr;
  double *t = nullptr, *y = nullptr, *G = nullptr, *tot = nullptr, *carry = nullptr, *pivot = nullptr, *grav = nullptr;
  SimuFrames f = {};
  unsigned char* run_buf = nullptr;               // lags, partials and results of a sweep: grows with the number of lags
  size_t run_bytes = 0;

  ~SimuDevice() {
    if (stream) (void)hipStreamSynchronize(stream);
    if (run_buf) (void)hipFree(run_buf);
    if (buf) (void)hipFree(buf);
    if (stream) (void)hipStreamDestroy(stream);
  }
  vc::SimuLog log() const { return vc::SimuLog{n, vc::simu_search_steps(n), t, y, G}; }

  void launch_prepare() {
    const dim3 grid(n_blocks, vc::kSeedImuChannels);
    hipLaunchKernelGGL(k_simu_totals, grid, dim3(256), 0, stream, t, y, n, n_blocks, tot);
    hipLaunchKernelGGL(k_simu_scan_totals, dim3(vc::kSeedImuChannels), dim3(256), 0, stream, tot, n_blocks, carry);
    hipLaunchKernelGGL(k_simu_scan, grid, dim3(256), 0, stream, t, y, n, n_blocks, carry, G);
    hipLaunchKernelGGL(k_simu_rates, dim3((n_int + 255) / 256), dim3(256), 0, stream, f, max_gap_s);
  }

  int open(int device, const vc::SeedImuData& d) {
    if (vch::open_device(device) != VC_OK) return VC_ERR_NO_DEVICE;
    n = d.n_samples; n_blocks = (n + kB - 1) / kB; n_frames = d.n_frames; n_int = n_frames - 1; chunks = vc::simu_chunks(n_int);
    max_gap_s = d.max_gap_s; min_valid = vc::simu_min_valid(d.min_intervals);
    const size_t N = (size_t)n, F = (size_t)n_frames;
    std::vector<double> h_y(6 * N);                                  // channel-major
    for (size_t k = 0; k < N; ++k)
      for (int c = 0; c < 3; ++c) { h_y[(size_t)c * N + k] = d.gyro[3 * k + c]; h_y[(size_t)(3 + c) * N + k] = d.accel[3 * k + c]; }
    double *d_ft = nullptr, *d_fq = nullptr;
    unsigned char* d_ok = nullptr;
    auto carve = [&](vch::Carver q) {
      t = q.take<double>(N); y = q.take<double>(6 * N); G = q.take<double>(6 * N); tot = q.take<double>(6 * (size_t)n_blocks);
      carry = q.take<double>(6 * (size_t)n_blocks); d_ft = q.take<double>(F); d_fq = q.take<double>(4 * F); d_ok = q.take<unsigned char>(F);
      f.a = q.take<double>(3 * (size_t)n_int + 3); f.inv_dt = q.take<double>((size_t)n_int); f.valid = q.take<unsigned char>((size_t)n_int);
      grav = q.take<double>(3 * (size_t)chunks);
      return q.bytes();
    };
    if (hipStreamCreate(&stream) != hipSuccess || hipMalloc((void**)&buf, carve(vch::Carver())) != hipSuccess) return VC_ERR_NO_DEVICE;
    carve(vch::Carver(buf));
    f.n_int = n_int; f.ft = d_ft; f.fq = d_fq; f.ok = d_ok;
    // the pivot: the rate of the first interval with one, in the rates' own array; without one, three zeros behind the array's end
    const int p = vc::simu_pivot_interval(d);
    pivot = f.a + 3 * (size_t)(p >= 0 ? p : n_int);
    f.pivot = pivot;
    bool ok = hipMemcpyAsync(t, d.imu_t, N * 8, hipMemcpyHostToDevice, stream) == hipSuccess &&
              hipMemcpyAsync(y, h_y.data(), 6 * N * 8, hipMemcpyHostToDevice, stream) == hipSuccess &&
              hipMemcpyAsync(d_ft, d.frame_t, F * 8, hipMemcpyHostToDevice, stream) == hipSuccess &&
              hipMemcpyAsync(d_fq, d.frame_q, 4 * F * 8, hipMemcpyHostToDevice, stream) == hipSuccess &&
              hipMemcpyAsync(d_ok, d.frame_ok, F, hipMemcpyHostToDevice, stream) == hipSuccess &&
              hipMemsetAsync(f.a + 3 * (size_t)n_int, 0, 24, stream) == hipSuccess;
    if (ok) { launch_prepare(); ok = hipGetLastError() == hipSuccess; }
    ok = hipStreamSynchronize(stream) == hipSuccess && ok;            // (h_y is read until here)
    return ok ? VC_OK : VC_ERR_NO_DEVICE;
  }

  struct RunArrays { double* lags; double* part; SimuOut o; };
  size_t carve_run(vch::Carver q, int n_lags, RunArrays* a) const {
    const size_t L = (size_t)n_lags;
    a->lags = q.take<double>(L); a->part = q.take<double>(L * (size_t)chunks * kM);
    a->o.J = q.take<double>(L); a->o.R = q.take<double>(9 * L); a->o.bias = q.take<double>(3 * L); a->o.count = q.take<int>(L); a->o.mom = q.take<double>(kM * L);
    return q.bytes();
  }
  int prepare_run(int n_lags, const double* lags, RunArrays* a) {
    const size_t need = carve_run(vch::Carver(), n_lags, a);
    if (need > run_bytes) {
      if (run_buf) (void)hipFree(run_buf);
      run_buf = nullptr; run_bytes = 0;
      if (hipMalloc((void**)&run_buf, need) != hipSuccess) return VC_ERR_NO_DEVICE;
      run_bytes = need;
    }
    carve_run(vch::Carver(run_buf), n_lags, a);
    if (hipMemcpyAsync(a->lags, lags, (size_t)n_lags * 8, hipMemcpyHostToDevice, stream) != hipSuccess) return VC_ERR_NO_DEVICE;
    return VC_OK;
  }
  void launch_sweep(const RunArrays& a, int n_lags) {
    for (int l0 = 0; l0 < n_lags; l0 += vc::kSeedImuMaxLags) {
      const int nl = n_lags - l0 < vc::kSeedImuMaxLags ? n_lags - l0 : vc::kSeedImuMaxLags;
      hipLaunchKernelGGL(k_simu_sweep, dim3(chunks, nl), dim3(256), 0, stream, log(), f, (const double*)a.lags, l0, chunks, a.part);
    }
    hipLaunchKernelGGL(k_simu_finish, dim3((n_lags + 255) / 256), dim3(256), 0, stream, (const double*)a.part, n_lags, chunks, (const double*)pivot, min_valid, a.o);
  }

  // the backend of vc::simu_pick; any output may be null
  int sweep(int n_lags, const double* lags, double* J, double* R, double* bias, int* count, double* mom) {
    RunArrays a;
    const int rc = prepare_run(n_lags, lags, &a);
    if (rc != VC_OK) return rc;
    launch_sweep(a, n_lags);
    const size_t L = (size_t)n_lags;
    auto down = [&](void* dst, const void* src, size_t bytes) { return !dst || hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, stream) == hipSuccess; };
    bool ok = hipGetLastError() == hipSuccess && down(J, a.o.J, L * 8) && down(R, a.o.R, L * 72) && down(bias, a.o.bias, L * 24) && down(count, a.o.count, L * 4) &&
              down(mom, a.o.mom, L * kM * 8);
    ok = hipStreamSynchronize(stream) == hipSuccess && ok;
    return ok ? VC_OK : VC_ERR_NO_DEVICE;
  }
  void launch_gravity(double lag, const double* R_ck) {
    SimuRot r;
    std::memcpy(r.r, R_ck, sizeof(r.r));
    hipLaunchKernelGGL(k_simu_gravity, dim3(chunks), dim3(256), 0, stream, log(), f, lag, r, grav);
  }
  int gravity(double lag, const double* R_ck, double* u) {
    std::vector<double> part(3 * (size_t)chunks);
    launch_gravity(lag, R_ck);
    if (hipGetLastError() != hipSuccess || hipMemcpyAsync(part.data(), grav, part.size() * 8, hipMemcpyDeviceToHost, stream) != hipSuccess ||
        hipStreamSynchronize(stream) != hipSuccess)
      return VC_ERR_NO_DEVICE;
    u[0] = u[1] = u[2] = 0.0;
    for (int c = 0; c < chunks; ++c)
      for (int k = 0; k < 3; ++k) u[k] += part[3 * (size_t)c + k];
    return VC_OK;
  }
};

int judge_data(const vc::SeedImuData& d) {
  if (!d.frame_t || !d.frame_q || !d.frame_ok || !d.imu_t || !d.gyro || !d.accel) return VC_ERR_BAD_ARG;
  if (d.n_frames < 2 || d.n_samples < 2) return VC_ERR_BAD_ARG;
  if (d.n_samples > vc::kSeedImuMaxN) return VC_ERR_UNSUPPORTED;      // (before anything is read)
  return vc::simu_data_ok(d) ? VC_OK : VC_ERR_BAD_ARG;
}

}  // namespace

extern "C" int vc_seed_imu_sweep(int device, int n_frames, const double* frame_t, const double* frame_q_wc, const unsigned char* frame_ok, int n_samples,
                                 const double* imu_t, const double* gyro, const double* accel, double max_gap_s, int min_intervals, int n_lags,
                                 const double* lags, double* J, double* R, double* bias, int* count, double* moments) {
  const vc::SeedImuData d{n_frames, frame_t, frame_q_wc, frame_ok, n_samples, imu_t, gyro, accel, max_gap_s, min_intervals};
  const int rc = judge_data(d);
  if (rc != VC_OK) return rc;
  if (!vc::simu_lags_ok(n_lags, lags)) return VC_ERR_BAD_ARG;
  SimuDevice dev;
  const int ro = dev.open(device, d);
  if (ro != VC_OK) return ro;
  return dev.sweep(n_lags, lags, J, R, bias, count, moments);
}

extern "C" int vc_seed_imu(int device, int n_frames, const double* frame_t, const double* frame_q_wc, const unsigned char* frame_ok, int n_samples,
                           const double* imu_t, const double* gyro, const double* accel, double max_gap_s, int min_intervals, double range_s, double step_s,
                           int fine, double* time_offset, double* R_ck, double* gyro_bias, double* g_dir, double* rms, double* signal, int* count, int* status,
                           int coarse_cap, double* coarse_lags, double* coarse_J, int* n_coarse) {
  const vc::SeedImuData d{n_frames, frame_t, frame_q_wc, frame_ok, n_samples, imu_t, gyro, accel, max_gap_s, min_intervals};
  if (!status || coarse_cap < 0) return VC_ERR_BAD_ARG;
  const int rc = judge_data(d);
  if (rc != VC_OK) return rc;
  if (!(range_s > 0.0) || !std::isfinite(range_s) || !std::isfinite(step_s) || fine < 1 || fine > vc::kSeedImuMaxLattice / 4) return VC_ERR_BAD_ARG;
  {                                                                   // (the lattice's size, judged before the device as in simu_pick)
    const double step = step_s > 0.0 ? step_s : vc::simu_median_step(n_samples, imu_t);
    if (!(std::floor(range_s / step + 1e-9) < 0.5 * vc::kSeedImuMaxLattice)) return VC_ERR_BAD_ARG;
  }
  SimuDevice dev;
  const int ro = dev.open(device, d);
  if (ro != VC_OK) return ro;
  vc::SeedImuResult r;
  const int rp = vc::simu_pick(dev, d, range_s, step_s, fine, &r);
  if (rp != VC_OK) return rp;
  *status = r.status;
  if (n_coarse) *n_coarse = r.n_coarse;
  const int n_copy = r.n_coarse < coarse_cap ? r.n_coarse : coarse_cap;
  if (coarse_lags) std::memcpy(coarse_lags, r.coarse_lags.data(), (size_t)n_copy * 8);
  if (coarse_J) std::memcpy(coarse_J, r.coarse_J.data(), (size_t)n_copy * 8);
  if (r.status != vc::kSeedImuOk) return VC_OK;                       // (nothing else is filled)
  if (time_offset) *time_offset = r.time_offset;
  if (R_ck) std::memcpy(R_ck, r.R_ck, 72);
  if (gyro_bias) std::memcpy(gyro_bias, r.gyro_bias, 24);
  if (g_dir) std::memcpy(g_dir, r.g_dir, 16);
  if (rms) *rms = r.rms;
  if (signal) *signal = r.signal;
  if (count) *count = r.count;
  return VC_OK;
}

extern "C" int vc_time_seed_imu(int device, int n_frames, const double* frame_t, const double* frame_q_wc, const unsigned char* frame_ok, int n_samples,
                                const double* imu_t, const double* gyro, const double* accel, double max_gap_s, int min_intervals, int n_lags,
                                const double* lags, int reps, double out_ms[3]) {
  const vc::SeedImuData d{n_frames, frame_t, frame_q_wc, frame_ok, n_samples, imu_t, gyro, accel, max_gap_s, min_intervals};
  if (reps < 1 || !out_ms) return VC_ERR_BAD_ARG;
  int rc = judge_data(d);
  if (rc != VC_OK) return rc;
  if (!vc::simu_lags_ok(n_lags, lags)) return VC_ERR_BAD_ARG;
  SimuDevice dev;
  rc = dev.open(device, d);
  if (rc != VC_OK) return rc;
  SimuDevice::RunArrays a;
  rc = dev.prepare_run(n_lags, lags, &a);
  if (rc != VC_OK) return rc;
  const double eye[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
  rc = vch::time_back_to_back(dev.stream, reps, [&]() { dev.launch_prepare(); }, &out_ms[0]);      // (the same input: the same bits)
  if (rc == VC_OK) rc = vch::time_back_to_back(dev.stream, reps, [&]() { dev.launch_sweep(a, n_lags); }, &out_ms[1]);
  if (rc == VC_OK) rc = vch::time_back_to_back(dev.stream, reps, [&]() { dev.launch_gravity(lags[0], eye); }, &out_ms[2]);
  return rc;
}
