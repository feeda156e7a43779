// vc_seed_rig.hip -- the rig seed (gfx950, wave64, fp64 throughout): the pose of every camera relative to camera 0 by a vote among the
// per-frame relative poses of every pair of cameras: vc_seed_rig, vc_time_seed_rig.  vc_seed_rig.hpp has the arithmetic and the tree.
//
// The host lists, per pair (a < b), the frames both cameras see, in frame order (only view_ok is read for that); pair p owns the entries
// off[p] .. off[p] + n[p] - 1 of every per-entry array, so a pair's data and the order of its sums do not depend on the other cameras.
//  k_srig_candidates   grid (tiles of 256 entries, pair), one lane per entry: X = T_aw T_bw^-1 and the scale d, 8 doubles.
//  k_srig_support      grid (tiles of 256 entries, pair): the N^2 part.  Every lane keeps candidate i in registers; the pair's candidates
//                      pass through a 16 KB LDS tile, 256 at a time, and every lane reads candidate j at the same address (a broadcast);
//                      the count is an integer.
//  k_srig_finish       one wavefront per pair: the largest support (the lowest entry among equals) by an integer butterfly, then two
//                      passes over the entries, lanes striding by entry: the refit over the winner's agreeing entries and the two spreads
//                      around it; the lane sums go through wave_allsum.
// Separate launches order the steps; no workgroup waits on another, no floating-point atomic, every loop's bound is known before the launch:
// two runs give the same bits, and a pair gives the same bits alone or among others.  No CPU fallback: without a device the entry points fail.
#include <hip/hip_runtime.h>
#include <cstring>
#include <vector>
#include "../../include/vicalib_amd.h"
#include "vc_device.h"
#include "vc_kutil.hpp"
#include "vc_hostutil.hpp"
#include "vc_seed_rig.hpp"

namespace {

constexpr int kT = vc::kSeedRigTile, kR = vc::kSeedRigRec;
static_assert(vc::kSeedRigMaxCams == vc::kMaxCams, "the rig seed serves the rigs the calibrator takes");
static_assert(kT == 256 && kR == 8, "one candidate per thread of a 256-thread workgroup, four 16-byte loads each");

struct SrigPair { int a, b, off, n; };

__device__ __forceinline__ void load_candidate(const double* __restrict__ c, double* X) {
  const vc::v4d lo = *reinterpret_cast<const vc::v4d*>(c), hi = *reinterpret_cast<const vc::v4d*>(c + 4);
  X[0] = lo.x; X[1] = lo.y; X[2] = lo.z; X[3] = lo.w; X[4] = hi.x; X[5] = hi.y; X[6] = hi.z; X[7] = hi.w;
}

__global__ __launch_bounds__(256) void k_srig_candidates(const SrigPair* __restrict__ pairs, int n_cams, const double* __restrict__ view_T,
                                                         const int* __restrict__ entry_frame, double* __restrict__ cand) {
  const SrigPair pr = pairs[blockIdx.y];
  const int e = blockIdx.x * kT + threadIdx.x;
  if (e >= pr.n) return;
  const size_t f = (size_t)entry_frame[pr.off + e];
  double Ta[7], Tb[7], X[kR];
#pragma unroll
  for (int k = 0; k < 7; ++k) { Ta[k] = view_T[(f * n_cams + pr.a) * 7 + k]; Tb[k] = view_T[(f * n_cams + pr.b) * 7 + k]; }
  vc::srig_candidate(Ta, Tb, X);
  double* o = cand + (size_t)(pr.off + e) * kR;
  *reinterpret_cast<vc::v4d*>(o) = vc::v4d{X[0], X[1], X[2], X[3]};
  *reinterpret_cast<vc::v4d*>(o + 4) = vc::v4d{X[4], X[5], X[6], X[7]};
}

__global__ __launch_bounds__(256) void k_srig_support(const SrigPair* __restrict__ pairs, const double* __restrict__ cand, double cos_half, double tol2,
                                                      int* __restrict__ support) {
  __shared__ __attribute__((aligned(32))) double tile[kT * kR];
  const SrigPair pr = pairs[blockIdx.y];
  const int n = pr.n, i0 = blockIdx.x * kT;
  if (i0 >= n) return;                                               // (the whole workgroup: before any barrier)
  const double* c = cand + (size_t)pr.off * kR;
  const int i = i0 + (int)threadIdx.x;
  double Xi[kR];
  load_candidate(c + (size_t)(i < n ? i : n - 1) * kR, Xi);           // (a lane behind the pair's end votes for the last entry and stores nothing)
  int count = 0;
  for (int j0 = 0; j0 < n; j0 += kT) {
    const int m = n - j0 < kT ? n - j0 : kT;
    __syncthreads();                                                 // (the previous tile has been read)
    if ((int)threadIdx.x < m) {
      const double* s = c + (size_t)(j0 + threadIdx.x) * kR;
      *reinterpret_cast<vc::v4d*>(tile + threadIdx.x * kR) = *reinterpret_cast<const vc::v4d*>(s);
      *reinterpret_cast<vc::v4d*>(tile + threadIdx.x * kR + 4) = *reinterpret_cast<const vc::v4d*>(s + 4);
    }
    __syncthreads();
#pragma unroll 4
    for (int j = 0; j < m; ++j) count += vc::srig_agree(Xi, tile + j * kR, cos_half, tol2) ? 1 : 0;
  }
  if (i < n) support[pr.off + i] = count;
}

struct SrigOut { double* T; double* rms; int* ints; };                // per pair: 7, 2 (degrees, metres), 3 (support, winner's frame, status)

__global__ __launch_bounds__(64) void k_srig_finish(const SrigPair* __restrict__ pairs, const double* __restrict__ cand, const int* __restrict__ support,
                                                    const int* __restrict__ entry_frame, double cos_half, double tol2, int min_support, SrigOut o) {
  const int p = blockIdx.x, lane = threadIdx.x;
  const SrigPair pr = pairs[p];
  const int n = pr.n;
  int* oi = o.ints + 3 * (size_t)p;
  if (n == 0) { if (lane == 0) oi[2] = vc::kSeedRigNoShared; return; }
  // the largest support, the lowest entry among equals: one integer key
  long long key = -1;
  for (int e = lane; e < n; e += 64) {
    const long long k = ((long long)support[pr.off + e] << 32) | (long long)(0x7fffffff - e);
    key = k > key ? k : key;
  }
#pragma unroll
  for (int s = 32; s > 0; s >>= 1) { const long long ok = __shfl_xor(key, s, 64); key = ok > key ? ok : key; }
  const int best = (int)(key >> 32), we = 0x7fffffff - (int)(key & 0xffffffffLL);
  if (best < min_support) { if (lane == 0) oi[2] = vc::kSeedRigFewSupport; return; }
  const double* c = cand + (size_t)pr.off * kR;
  double W[kR], acc[7] = {0, 0, 0, 0, 0, 0, 0};
  load_candidate(c + (size_t)we * kR, W);
  int cnt = 0;
  for (int e = lane; e < n; e += 64) {
    double X[kR];
    load_candidate(c + (size_t)e * kR, X);
    if (vc::srig_agree(W, X, cos_half, tol2)) { vc::srig_refit_term(W, X, acc); ++cnt; }
  }
  cnt = vc::wave_allsum(cnt);                                        // (= best: the same test on the same operands)
#pragma unroll
  for (int k = 0; k < 7; ++k) acc[k] = vc::wave_allsum(acc[k]);
  double T[7], a2 = 0.0, d2 = 0.0, rms_deg, rms_m;
  vc::srig_refit_finish(acc, cnt, T);
  for (int e = lane; e < n; e += 64) {
    double X[kR];
    load_candidate(c + (size_t)e * kR, X);
    if (vc::srig_agree(W, X, cos_half, tol2)) vc::srig_spread_term(T, X, &a2, &d2);
  }
  a2 = vc::wave_allsum(a2); d2 = vc::wave_allsum(d2);
  vc::srig_spread_finish(a2, d2, cnt, &rms_deg, &rms_m);
  if (lane == 0) {
#pragma unroll
    for (int k = 0; k < 7; ++k) o.T[7 * (size_t)p + k] = T[k];
    o.rms[2 * (size_t)p] = rms_deg; o.rms[2 * (size_t)p + 1] = rms_m;
    oi[0] = cnt; oi[1] = entry_frame[pr.off + we]; oi[2] = vc::kSeedRigOk;
  }
}

// The data of one call on the device.  Not a handle of the C ABI: it lives for one entry point.
struct SrigDevice {
  vc::SrigIndex ix;
  vc::SrigTol tol = {};
  int n_cams = 0, min_support = 1;
  hipStream_t stream = nullptr;
  unsigned char* buf = nullptr;
  SrigPair* pairs = nullptr;
  double *view_T = nullptr, *cand = nullptr;
  int *entry_frame = nullptr, *support = nullptr;
  SrigOut o = {};

  ~SrigDevice() {
    if (stream) (void)hipStreamSynchronize(stream);
    if (buf) (void)hipFree(buf);
    if (stream) (void)hipStreamDestroy(stream);
  }
  bool any() const { return ix.n_max > 0; }

  int open(int device, int n_frames, int n_cams_, const unsigned char* view_ok, const double* view_T_cw, double tol_deg, int min_support_) {
    if (vch::open_device(device) != VC_OK) return VC_ERR_NO_DEVICE;
    n_cams = n_cams_; min_support = min_support_; tol = vc::srig_tol(tol_deg);
    vc::srig_build_index(n_frames, n_cams, view_ok, &ix);
    if (!any()) return VC_OK;                                         // (no pair shares a frame: nothing to launch)
    const size_t E = ix.frame.size(), P = (size_t)ix.n_pairs, V = (size_t)n_frames * n_cams * 7;
    auto carve = [&](vch::Carver q) {
      pairs = q.take<SrigPair>(P); view_T = q.take<double>(V); cand = q.take<double>(E * kR); entry_frame = q.take<int>(E); support = q.take<int>(E);
      o.T = q.take<double>(7 * P); o.rms = q.take<double>(2 * P); o.ints = q.take<int>(3 * P);
      return q.bytes();
    };
    if (hipStreamCreate(&stream) != hipSuccess || hipMalloc((void**)&buf, carve(vch::Carver())) != hipSuccess) return VC_ERR_NO_DEVICE;
    carve(vch::Carver(buf));
    SrigPair hp[vc::kSeedRigMaxPairs];
    for (int p = 0; p < ix.n_pairs; ++p) hp[p] = SrigPair{ix.a[p], ix.b[p], ix.off[p], ix.n[p]};
    bool ok = hipMemcpyAsync(pairs, hp, P * sizeof(SrigPair), hipMemcpyHostToDevice, stream) == hipSuccess &&
              hipMemcpyAsync(view_T, view_T_cw, V * 8, hipMemcpyHostToDevice, stream) == hipSuccess &&      // (a view that is not ok travels and is never read)
              hipMemcpyAsync(entry_frame, ix.frame.data(), E * 4, hipMemcpyHostToDevice, stream) == hipSuccess;
    ok = hipStreamSynchronize(stream) == hipSuccess && ok;            // (hp is read until here)
    return ok ? VC_OK : VC_ERR_NO_DEVICE;
  }
  dim3 grid() const { return dim3((ix.n_max + kT - 1) / kT, ix.n_pairs); }
  void launch_candidates() { hipLaunchKernelGGL(k_srig_candidates, grid(), dim3(256), 0, stream, (const SrigPair*)pairs, n_cams, (const double*)view_T, (const int*)entry_frame, cand); }
  void launch_support() { hipLaunchKernelGGL(k_srig_support, grid(), dim3(256), 0, stream, (const SrigPair*)pairs, (const double*)cand, tol.cos_half, tol.tol2, support); }
  void launch_finish() {
    hipLaunchKernelGGL(k_srig_finish, dim3(ix.n_pairs), dim3(64), 0, stream, (const SrigPair*)pairs, (const double*)cand, (const int*)support, (const int*)entry_frame,
                       tol.cos_half, tol.tol2, min_support, o);
  }
};

bool outputs_ok(const double* pair_T_ab, const int* pair_shared, const int* pair_support, const int* pair_winner, const double* pair_rms_deg, const double* pair_rms_m,
                const int* pair_status, const double* cam_T_c0, const int* cam_parent, const int* cam_status) {
  return pair_T_ab && pair_shared && pair_support && pair_winner && pair_rms_deg && pair_rms_m && pair_status && cam_T_c0 && cam_parent && cam_status;
}

}  // namespace

extern "C" int vc_seed_rig(int device, int n_frames, int n_cams, const unsigned char* view_ok, const double* view_T_cw, double tol_deg, int min_support,
                           double* pair_T_ab, int* pair_shared, int* pair_support, int* pair_winner, double* pair_rms_deg, double* pair_rms_m, int* pair_status,
                           double* cam_T_c0, int* cam_parent, int* cam_status) {
  const int rc = vc::srig_judge(n_frames, n_cams, view_ok, view_T_cw, tol_deg, min_support,
                                outputs_ok(pair_T_ab, pair_shared, pair_support, pair_winner, pair_rms_deg, pair_rms_m, pair_status, cam_T_c0, cam_parent, cam_status));
  if (rc != 0) return rc == -7 ? VC_ERR_UNSUPPORTED : VC_ERR_BAD_ARG;
  SrigDevice dev;
  const int ro = dev.open(device, n_frames, n_cams, view_ok, view_T_cw, tol_deg, min_support);
  if (ro != VC_OK) return ro;
  const int P = dev.ix.n_pairs;
  std::vector<double> T(7 * (size_t)P + 1), rms(2 * (size_t)P + 1);
  std::vector<int> ints(3 * (size_t)P + 1, vc::kSeedRigNoShared);
  if (dev.any()) {
    dev.launch_candidates(); dev.launch_support(); dev.launch_finish();
    bool ok = hipGetLastError() == hipSuccess && hipMemcpyAsync(T.data(), dev.o.T, 7 * (size_t)P * 8, hipMemcpyDeviceToHost, dev.stream) == hipSuccess &&
              hipMemcpyAsync(rms.data(), dev.o.rms, 2 * (size_t)P * 8, hipMemcpyDeviceToHost, dev.stream) == hipSuccess &&
              hipMemcpyAsync(ints.data(), dev.o.ints, 3 * (size_t)P * 4, hipMemcpyDeviceToHost, dev.stream) == hipSuccess;
    ok = hipStreamSynchronize(dev.stream) == hipSuccess && ok;
    if (!ok) return VC_ERR_NO_DEVICE;
  }
  std::vector<int> status((size_t)P + 1), supp((size_t)P + 1, 0);
  std::vector<double> Tab(7 * (size_t)P + 1, 0.0);
  for (int p = 0; p < P; ++p) {
    status[p] = ints[3 * (size_t)p + 2];
    pair_shared[p] = dev.ix.n[p]; pair_status[p] = status[p];
    if (status[p] != vc::kSeedRigOk) continue;                        // (the other outputs of a refused pair stay as they were)
    supp[p] = ints[3 * (size_t)p];
    std::memcpy(&Tab[7 * (size_t)p], &T[7 * (size_t)p], 56);
    std::memcpy(pair_T_ab + 7 * (size_t)p, &T[7 * (size_t)p], 56);
    pair_support[p] = supp[p]; pair_winner[p] = ints[3 * (size_t)p + 1];
    pair_rms_deg[p] = rms[2 * (size_t)p]; pair_rms_m[p] = rms[2 * (size_t)p + 1];
  }
  double cam_T[7 * vc::kSeedRigMaxCams];
  vc::srig_tree(n_cams, status.data(), supp.data(), Tab.data(), cam_T, cam_parent, cam_status);
  for (int c = 0; c < n_cams; ++c)
    if (cam_status[c] == vc::kSeedRigReached) std::memcpy(cam_T_c0 + 7 * (size_t)c, cam_T + 7 * (size_t)c, 56);
  return VC_OK;
}

extern "C" int vc_time_seed_rig(int device, int n_frames, int n_cams, const unsigned char* view_ok, const double* view_T_cw, double tol_deg, int min_support, int reps,
                                double kernel_ms[3]) {
  if (reps < 1) return VC_ERR_BAD_ARG;
  int rc = vc::srig_judge(n_frames, n_cams, view_ok, view_T_cw, tol_deg, min_support, kernel_ms != nullptr);
  if (rc != 0) return rc == -7 ? VC_ERR_UNSUPPORTED : VC_ERR_BAD_ARG;
  SrigDevice dev;
  rc = dev.open(device, n_frames, n_cams, view_ok, view_T_cw, tol_deg, min_support);
  if (rc != VC_OK) return rc;
  kernel_ms[0] = kernel_ms[1] = kernel_ms[2] = 0.0;
  if (!dev.any()) return VC_OK;
  rc = vch::time_back_to_back(dev.stream, reps, [&]() { dev.launch_candidates(); }, &kernel_ms[0]);      // (the same input: the same bits)
  if (rc == VC_OK) rc = vch::time_back_to_back(dev.stream, reps, [&]() { dev.launch_support(); }, &kernel_ms[1]);
  if (rc == VC_OK) rc = vch::time_back_to_back(dev.stream, reps, [&]() { dev.launch_finish(); }, &kernel_ms[2]);
  return rc;
}
