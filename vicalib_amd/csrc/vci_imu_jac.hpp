// vci_imu_jac.hpp -- k_imu_jac: half a wavefront per IMU block; lane = local column of the block, carried as a dual number through the
// application of the block's delta to the start state and the residual's tail -- the lane-parallel form of ceres::Jet<double,35>
// (vc_imu.hpp, "delta form"); then Cauchy(100) weight and the 33 x 33 weighted J^T J / J^T r of the block.
// Kernel fragment of vc_imu_kernels.hip alone (defines __global__ symbols; included there in stage order; not for host harnesses).
#pragma once
#include <hip/hip_runtime.h>
#include "vc_math.hpp"
#include "vc_imu.hpp"
#include "vc_device.h"
#include "vc_kutil.hpp"

namespace vc {

// ------------------------------------------------------------------------------------------ IMU Jacobian
constexpr int kImuJacLds = 34 * 9 + 6;            // [34][9]: the block's 33 local columns and, as a 34th, the residual itself
// Where the block's J^T J on the matrix pipe (round 6) lands in the compact block record (vc_device.h: kSeg*, seg_entry: entry e -> row a, column b;
// b = 33: gradient): the 34 columns (33 local columns + the residual) are three column tiles of 16; tile pair (I, J) of v_mfma_f64_16x16x4 leaves
// entry (a, b) = (16 I + 4 g + lane / 16, 16 J + lane % 16) in accumulator register g of `lane` -- v[I * 3 + J][lane][g] is that entry's place in
// the compact record (0xffff: the record has no such entry)
struct SegInv {
  unsigned short v[9][64][4];
  constexpr SegInv() : v() {
    for (int t = 0; t < 9; ++t) for (int l = 0; l < 64; ++l) for (int g = 0; g < 4; ++g) v[t][l][g] = 0xffff;
    for (int e = 0; e < kSegLen; ++e) {
      int a = 0, b = 0; seg_entry(e, &a, &b);
      const int I = a / 16, J = b / 16, rt = a % 16;
      v[I * 3 + J][(rt % 4) * 16 + b % 16][rt / 4] = (unsigned short)e;
    }
  }
};
__constant__ SegInv d_seg_inv = SegInv();
// The sweep proper.  Two IMU blocks per wavefront, lane = local column of the block: frame j's pose (6), frame j-1's pose (6) and
// velocity (3), gravity (2), biases (6), scale factors (6), time offset -- 30 lanes put the block's delta on the start state and
// run the residual's tail under one dual direction each (vc_imu.hpp: imu_block_final_direction); the three columns of frame j's
// velocity are -W^T rows 6..8, written directly.  Then Cauchy(100) weight and the 33 x 33 weighted J^T J / J^T r of the block.
// trial = 0: at the accepted state, when the control record asks for a linearisation; trial = 1: at the trial state into buffer
// 1 - cur (cost = the block's trial cost; the blocks are the next linearisation if the step is accepted) -- see k_reproj_jac.
// phase stamps of the first wavefront (profiling builds only, -DVC_IJ_STAMPS): 100 MHz s_memrealtime ticks in dbg[0..7]
#ifdef VC_IJ_STAMPS
#define IJSTAMP(i) do { if (blockIdx.x == 0 && threadIdx.x == 0) v.dbg[i] = (long long)__builtin_amdgcn_s_memrealtime(); } while (0)
#else
#define IJSTAMP(i) do { } while (0)
#endif
__global__ __launch_bounds__(256) void k_imu_jac(DevView v, int wr, int trial) {
  __shared__ double sh[8 * kImuJacLds];
  __shared__ double s_wq[8 * 84];                  // the block's 9 x 9 weight, staged once (round 6: every lane loaded all 81 entries itself)
  // (round 6 also tried requesting everything ahead of the control record -- the two frames' states and the gravity record of BOTH state
  //  buffers, one value per lane, the buffer in use to LDS --: 23.1 us against 21.4 on the same box, reverted)
  IJSTAMP(0);
  // (vc_kutil.hpp: a void pass's trial kernels may run ahead of the previous decision -- nothing stored, not counted either: k_final of a
  //  void pass does not wait for the counts)
  if (trial && v.sync_seq > 0 && workgroup_pass_void(v)) return;
  const Ctrl* ct = v.ctrl;
  if (ct->done || (!trial && !ct->need_lin)) {
    // (a finished solve: the workgroup still counts itself in the second count -- k_final of this pass waits for it, so that the main
    //  stream never runs ahead of this one into the next solve)
    if (trial && v.final_wait > 0 && threadIdx.x == 0) __hip_atomic_fetch_add(v.sync_flags + 11, 1LL, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    return;
  }
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int half = lane >> 5, l = lane & 31;
  const int n_blocks = v.n_frames - 1;
  const int s_raw = (blockIdx.x * 4 + wave) * 2 + half;       // block s couples frames s -> s+1
  const bool exists = s_raw < n_blocks;
  const int s = exists ? s_raw : n_blocks - 1;                 // a half past the end shadows the last block and stores nothing
  const int cur = trial ? 1 - ct->cur : ct->cur, j = s + 1;
  double* Jl = sh + (wave * 2 + half) * kImuJacLds;            // [34][9] local columns: cur9 | prev9 | imu15 | residual
  const double* T2 = v.poses[cur] + (size_t)j * kPoseStride;
  const double* T1 = v.poses[cur] + (size_t)(j - 1) * kPoseStride;
  const double* v2 = v.vel[cur] + (size_t)j * 4;
  const double* v1 = v.vel[cur] + (size_t)(j - 1) * 4;
  const double* wq_g = v.wsqrtb[wr] + (size_t)s * 81;
  double* wq = s_wq + (wave * 2 + half) * 84;
  {
    double t3[3];
#pragma unroll
    for (int t = 0; t < 3; ++t) { const int idx = l + 32 * t; t3[t] = wq_g[idx < 81 ? idx : 0]; }
#pragma unroll
    for (int t = 0; t < 3; ++t) { const int idx = l + 32 * t; if (idx < 81) wq[idx] = t3[t]; }
  }
  const double* brec = v.imu_delta_blk + (size_t)s * kBlockDeltaStride;
  double r[9], dr[9];
  const int col = (l < 6) ? l : (l < 30 ? l + 3 : -1);         // lanes 30, 31 carry the values only
  const bool valid = brec[10] >= 0.0;
  unsigned long long seg_at[9];      // where the lane's four accumulator entries of every tile pair go in the record (tile pair (2, 0) has none)
#pragma unroll
  for (int t = 0; t < 9; ++t) seg_at[t] = t == 6 ? ~0ull : *reinterpret_cast<const unsigned long long*>(&d_seg_inv.v[t][lane][0]);
  wave_lds_sync();
  IJSTAMP(1);
  imu_block_final_direction(valid, brec, wq, v.rotation_only, T2, T1, v2, v1, v.imu_grav + cur * 16, col, r, dr);
  IJSTAMP(2);
  if (col >= 0) {
#pragma unroll
    for (int k = 0; k < 9; ++k) Jl[col * 9 + k] = dr[k];
  }
  if (l < 3) {                                                 // frame j's velocity: r = W^T raw, raw[6 + l] = v_pred - v2
#pragma unroll
    for (int k = 0; k < 9; ++k) {
      const bool zeroed = v.rotation_only && (k < 3 || k >= 6);
      Jl[(6 + l) * 9 + k] = (valid && !zeroed) ? -wq[(6 + l) * 9 + k] : 0.0;
    }
  }
  if (l == 31) {                                               // the residual rides as a 34th column: J^T r = its products with the others
#pragma unroll
    for (int k = 0; k < 9; ++k) Jl[33 * 9 + k] = r[k];
  }
  wave_lds_sync();
  double ss = 0.0;
#pragma unroll
  for (int k = 0; k < 9; ++k) ss += r[k] * r[k];
  double rho, rho1;
  loss_cauchy100(ss, &rho, &rho1);
  const double w = ct->imu_mult * rho1;
  if (trial) {                 // the workgroup's share of the trial cost (8 blocks, fixed order); all threads reach this barrier
    __shared__ double s_cost[8];
    if (l == 0) s_cost[wave * 2 + half] = exists ? ct->imu_mult * rho : 0.0;
    __syncthreads();
    if (threadIdx.x == 0) {
      const double wc = ((s_cost[0] + s_cost[1]) + (s_cost[2] + s_cost[3])) + ((s_cost[4] + s_cost[5]) + (s_cost[6] + s_cost[7]));
      if (v.final_wait > 0) {
        // flag hand-overs: k_final (main stream) takes the trial cost as soon as every workgroup has delivered its share -- a
        // device-coherent store and a count, no cache write-back -- and decides while this kernel still writes its records
        // (round 6 tried moving the count behind this thread's record stores -- the store's acknowledgement holds wavefront 0 back by
        //  ~2 us here: the kernel ended 1.2 us earlier and k_final 3.2 us later behind it; reverted)
        __hip_atomic_store(v.wg_imu_trial + blockIdx.x, wc, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __builtin_amdgcn_s_waitcnt(0);          // the store has been performed before the count moves
        __hip_atomic_fetch_add(v.sync_flags + 4, 1LL, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      } else v.wg_imu_trial[blockIdx.x] = wc;
    }
  }
  IJSTAMP(3);
  // flag hand-overs, trial sweep: the records go out as device-coherent stores and the workgroup counts itself a second time once they
  // have been performed -- k_final ends on that count (round 4: on a flag a one-thread kernel raised behind this one, 6 us after this
  // kernel's end, which since round 5's leaner k_final was what the pass ended on)
  const bool counted2 = trial && v.final_wait > 0;
  // J^T J and J^T r of the block in the compact record, entry e = w * <column a, column b> with the residual as column 33 -- on the matrix
  // pipe (round 6).  As 25 nine-term dot products per lane the phase was 450 LDS reads per lane, 6.2 of the kernel's ~20 us; here the whole
  // wavefront takes its two blocks one after the other: the block's [34][9] image read ONCE as nine operand registers (column tile T, rows
  // 4 ks .. 4 ks + 3: the same register is the A operand of tile pairs (T, .) and the B operand of (., T)), 8 tile pairs x 3 k-steps of
  // v_mfma_f64_16x16x4, and every accumulator entry goes to the place the inverse table names.  (a, b) and (b, a) are the same products in
  // the same order: the record's symmetric blocks stay symmetric to the bit.  (The dot-product form, rounds 1-5, asked for its 25 (row, column)
  // pairs per lane at the kernel's entry, statically unrolled: as a loop every entry waited for its own table look-up -- 25 dependent global
  // round trips, 10 of the kernel's 24 us at cfg3.)
  {
    const int i16 = lane & 15, kq = lane >> 4;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      if (!__builtin_amdgcn_readlane((int)exists, 32 * h)) continue;               // (wave-uniform)
      const double wh = readlane_f64(w, 32 * h);
      const int sb = __builtin_amdgcn_readlane(s, 32 * h);
      const double* Jb = sh + (wave * 2 + h) * kImuJacLds;
      double op[3][3];
#pragma unroll
      for (int T = 0; T < 3; ++T)
#pragma unroll
        for (int ks = 0; ks < 3; ++ks) {
          const int c = 16 * T + i16, rr = 4 * ks + kq;
          const bool in = c < 34 && rr < 9;
          const double x = Jb[in ? c * 9 + rr : 0];
          op[T][ks] = in ? x : 0.0;
        }
      double* rec = v.segb[cur] + (size_t)sb * kSegStride;
#pragma unroll
      for (int I = 0; I < 3; ++I)
#pragma unroll
        for (int J = 0; J < 3; ++J) {
          if (I == 2 && J == 0) continue;
          v4d acc = (v4d){0.0, 0.0, 0.0, 0.0};
#pragma unroll
          for (int ks = 0; ks < 3; ++ks) acc = __builtin_amdgcn_mfma_f64_16x16x4f64(op[I][ks], op[J][ks], acc, 0, 0, 0);
          const unsigned long long at = seg_at[I * 3 + J];
#pragma unroll
          for (int g = 0; g < 4; ++g) {
            const unsigned e = (unsigned)(at >> (16 * g)) & 0xffffu;
            if (e != 0xffffu) { if (counted2) __hip_atomic_store(rec + e, wh * acc[g], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); else rec[e] = wh * acc[g]; }
          }
        }
    }
    if (exists && l == 0) { if (counted2) __hip_atomic_store(v.seg_costb[cur] + s, ct->imu_mult * rho, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); else v.seg_costb[cur][s] = ct->imu_mult * rho; }
  }
  if (counted2) {
    __builtin_amdgcn_s_waitcnt(0);          // this wavefront's stores have been performed
    __syncthreads();
    if (threadIdx.x == 0) __hip_atomic_fetch_add(v.sync_flags + 11, 1LL, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  IJSTAMP(4);
}

}  // namespace vc
