// vci_imu_block.hpp -- k_imu_block: the part of the preintegration that does not depend on any pose, one wavefront per block: eight lanes per
// dual direction (gyro biases / scale factors, time offset; accelerometer parameters analytically beside them), lane = two sample intervals
// (RK4 steps from the identity state), inclusive DPP scan over the eight lanes.
// Kernel fragment of vc_imu_kernels.hip alone (defines __global__ symbols; included there in stage order; not for host harnesses).
#pragma once
#include <hip/hip_runtime.h>
#include "vc_math.hpp"
#include "vc_imu.hpp"
#include "vc_device.h"
#include "vc_kutil.hpp"
#include "vci_lanes.hpp"

namespace vc {

// ------------------------------------------------------------------------------------------ IMU block deltas
// The pose-independent half of the IMU sweep (vc_imu.hpp, "delta form") in one launch, nothing but the block records written: the
// interval deltas never leave the registers (round 3 wrote a 1120-byte record per sample interval with k_imu_delta and read it
// straight back with k_imu_block: 53 of the sweep's 73 MB per pass at BASELINE cfg3, behind a chain of ~12 dependent appends per
// block).  ONE WAVEFRONT PER IMU BLOCK, eight groups of eight lanes:
//   group g = 0..5   dual direction = gyro bias / scale factor g, and beside it -- no dual number needed, the velocity and position
//                    deltas are linear in the accelerometer inputs -- the partials along accelerometer bias / scale factor g;
//   group 6          dual direction = time offset (moves the interpolated end samples and the end intervals' lengths);
//   group 7          spare (shadows group 6, stores nothing);  the values ride in every group, group 0 stores them.
// Lane l of a group takes sample intervals 2 l + 1 and 2 l + 2 of the block (vc_imu.hpp: imu_interval_delta_ga, the RK4 step from
// the identity state written out) and appends the second to the first; an inclusive scan over the group's eight lanes (composition is
// associative; DPP row shifts, three levels, no LDS) leaves the block's delta in lane 7.  Blocks with more than 16 intervals run in
// rounds, lane 7 appending the rounds' totals (kept in LDS between rounds).  Round 4's first cut had one lane per (interval,
// record column) -- 14 x 16 lanes, 3.5 wavefronts per block, every lane repeating the values under its own direction and the scan
// costing as much as the steps: 57 us at cfg3 against 53 for the two kernels it replaced; this form runs a quarter of the wavefronts.
// Depends on the shared IMU parameters only: in a solve it runs behind the reduced solve, next to the chain's back-substitution.
// An empty sample range is flagged by T = -1 in the record.
// an IntervalDeltaT (vc_imu.hpp) as kDtDoubles doubles: values Q P V T | tangent dth dp dv dt | ap | av
__device__ __forceinline__ void delta_t_pack(const IntervalDeltaT& X, double* f) {
#pragma unroll
  for (int k = 0; k < 4; ++k) f[k] = X.d.q[k];
#pragma unroll
  for (int k = 0; k < 3; ++k) { f[4 + k] = X.d.p[k]; f[7 + k] = X.d.v[k]; f[11 + k] = X.dth[k]; f[14 + k] = X.dp[k]; f[17 + k] = X.dv[k]; f[21 + k] = X.ap[k]; f[24 + k] = X.av[k]; }
  f[10] = X.d.t; f[20] = X.dt;
}
__device__ __forceinline__ void delta_t_unpack(const double* f, IntervalDeltaT* X) {
#pragma unroll
  for (int k = 0; k < 4; ++k) X->d.q[k] = f[k];
#pragma unroll
  for (int k = 0; k < 3; ++k) { X->d.p[k] = f[4 + k]; X->d.v[k] = f[7 + k]; X->dth[k] = f[11 + k]; X->dp[k] = f[14 + k]; X->dv[k] = f[17 + k]; X->ap[k] = f[21 + k]; X->av[k] = f[24 + k]; }
  X->d.t = f[10]; X->dt = f[20];
}
template <int N> __device__ __forceinline__ void delta_t_scan_level(IntervalDeltaT* X, int l) {
  double f[kDtDoubles];
  delta_t_pack(*X, f);
#pragma unroll
  for (int k = 0; k < kDtDoubles; ++k) f[k] = row_shr<N>(f[k], f[k]);
  IntervalDeltaT A;
  delta_t_unpack(f, &A);
  imu_delta_t_then(&A, *X);
  if (l >= N) *X = A;                            // (the first N lanes of a group have no partner: what the shift brought them belongs to the group below)
}
// phase stamps of one wavefront in the middle of the grid (profiling builds only, -DVC_IB_STAMPS): 100 MHz s_memrealtime ticks in dbg[0..9]
#ifdef VC_IB_STAMPS
#define IBSTAMP(i) do { if (blockIdx.x == gridDim.x / 2 && threadIdx.x == 0) v.dbg[i] = (long long)__builtin_amdgcn_s_memrealtime(); } while (0)
#else
#define IBSTAMP(i) do { } while (0)
#endif
#ifndef VC_IMU_BLOCK_WAVES
#define VC_IMU_BLOCK_WAVES 2
#endif
#ifdef VC_IMU_BLOCK_EU      // (A/B builds: a register budget of 512 / n per wavefront -- n = 3: 168 registers, 268 B of scratch)
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(VC_IMU_BLOCK_EU, VC_IMU_BLOCK_EU))) void k_imu_block(DevView v, int trial) {
#else
__global__ __launch_bounds__(256, VC_IMU_BLOCK_WAVES) void k_imu_block(DevView v, int trial) {
#endif
  __shared__ double s_carry[32 * kDtDoubles];
  // the first interval's delta while the second is formed: tangent and accelerometer partials per lane (16 doubles), the VALUES once per
  // interval -- they are the same numbers in all eight groups, group 0 writes them: 42 KB per workgroup with the carry, not 62: two
  // workgroups fit a CU's LDS beside a workgroup of the back-substitution (68 KB at BASELINE cfg3).  (Its registers then hold the grid to
  // one workgroup per CU there -- 252 + 216 of a SIMD's 512 -- and two rounds; a step under ~144 registers spills: HISTORY round 6)
  __shared__ double s_park[256 * (kDtDoubles - 11)];
  __shared__ double s_parkv[4 * 8 * 11];
  IBSTAMP(0);
  if (trial && v.sync_seq > 0 && workgroup_pass_void(v)) return;      // (vc_kutil.hpp: a void pass's trial kernels may run ahead of the previous decision)
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);      // (scalar: everything per block stays out of the vector registers)
  const int g = lane >> 3, l = lane & 7;
  const int n_blocks = v.n_frames - 1;
  const int s_raw = blockIdx.x * 4 + wave;                             // block s couples frames s -> s + 1
  const int s = s_raw < n_blocks ? s_raw : n_blocks - 1;               // (a wavefront past the end shadows the last block and stores nothing)
  // requested together with the control record, not behind it (a wavefront's life is a chain of dependent memory round trips -- control
  // record, time offset, sample range, samples: ~7 of its 14 us; this is one of them): the frame times and the time offset of BOTH buffers
  const double toff0 = v.imus[0][14], toff1 = v.imus[1][14];
  const double t_start = v.frame_time[s], t_end = v.frame_time[s + 1];
  const Ctrl* ct = v.ctrl;
  const int c_done = ct->done, c_need = ct->need_lin, c_cur = ct->cur;
  if (c_done || (!trial && !c_need)) return;
  IBSTAMP(1);
  const int cur = trial ? 1 - c_cur : c_cur;
  const double* im = v.imus[cur];
  const double toff = cur ? toff1 : toff0;
  const ImuView buf = imu_view(v);
  ImuRange rg = imu_range_lanes(buf, t_start, t_end, toff, lane);
  rg.valid = __builtin_amdgcn_readfirstlane(rg.valid); rg.i0 = __builtin_amdgcn_readfirstlane(rg.i0); rg.i1 = __builtin_amdgcn_readfirstlane(rg.i1);
  rg.k0 = __builtin_amdgcn_readfirstlane(rg.k0); rg.k1 = __builtin_amdgcn_readfirstlane(rg.k1);
  rg.first_end = __builtin_amdgcn_readfirstlane(rg.first_end); rg.last_end = __builtin_amdgcn_readfirstlane(rg.last_end);
  double* rec = v.imu_delta_blk + (size_t)s * kBlockDeltaStride;
  IBSTAMP(2);
  if (rg.valid) {                                                      // (wave-uniform)
    const int n_int = (rg.k1 - rg.k0 + 1) + 1;                         // intervals between the n_int + 1 range elements
    const int gsel = g < 7 ? g : 6;
    double* cr = s_carry + (threadIdx.x >> 3) * kDtDoubles;
    IntervalDeltaT X;
#pragma unroll 1
    for (int base = 0; base < n_int; base += 16) {
      {
        // the first interval's delta waits in LDS while the second is formed (27 doubles that would otherwise sit -- or spill --
        // under the second RK4 step); a loop that is not unrolled: one copy of the step, nothing of the second interval scheduled
        // into the first
        IntervalDeltaT Y;
        double* pk = s_park + threadIdx.x;
        double* pv = s_parkv + (wave * 8 + l) * 11;
#pragma unroll 1
        for (int half = 0; half < 2; ++half) {
          // (the group index made opaque per iteration: otherwise everything the step derives from it -- seed masks, unit vector,
          //  selects -- is hoisted out of the loops and sits in registers across both steps and the scan)
          int gs = gsel;
          asm volatile("" : "+v"(gs));
          imu_interval_delta_t(buf, rg, mk(toff, gs == 6 ? 1.0 : 0.0), t_start, t_end, base + 2 * l + 1 + half, n_int, im + 2, im + 8, gs, &Y);
          IBSTAMP(3 + half);
          if (half == 0) {
            double f[kDtDoubles];
            delta_t_pack(Y, f);
#pragma unroll
            for (int k = 11; k < kDtDoubles; ++k) pk[(k - 11) * 256] = f[k];
            if (g == 0) {
#pragma unroll
              for (int k = 0; k < 11; ++k) pv[k] = f[k];
            }
          }
        }
        wave_lds_sync_local();               // (group 0's values are read by the other groups' lanes)
        double f[kDtDoubles];
#pragma unroll
        for (int k = 0; k < 11; ++k) f[k] = pv[k];
#pragma unroll
        for (int k = 11; k < kDtDoubles; ++k) f[k] = pk[(k - 11) * 256];
        delta_t_unpack(f, &X);
        wave_lds_sync_local();               // (... before the next round's first interval overwrites them)
        imu_delta_t_then(&X, Y);
      }
      IBSTAMP(5);
      delta_t_scan_level<1>(&X, l); delta_t_scan_level<2>(&X, l); delta_t_scan_level<4>(&X, l);
      IBSTAMP(6);
      if (l == 7) {                                                    // the round's total; the rounds before it rest in LDS
        if (base > 0) {
          IntervalDeltaT A;
          double f[kDtDoubles];
#pragma unroll
          for (int k = 0; k < kDtDoubles; ++k) f[k] = cr[k];
          delta_t_unpack(f, &A);
          imu_delta_t_then(&A, X);
          X = A;
        }
        if (base + 16 < n_int) {
          double f[kDtDoubles];
          delta_t_pack(X, f);
#pragma unroll
          for (int k = 0; k < kDtDoubles; ++k) cr[k] = f[k];
        }
      }
    }
    if (l == 7 && s_raw < n_blocks) imu_block_record_store(X, g, rec);
    IBSTAMP(7);
  } else if (lane == 0 && s_raw < n_blocks) rec[10] = -1.0;
  // the gravity record of this state for k_imu_jac (one lane of the spare group)
  if (blockIdx.x == 0 && threadIdx.x == 63) imu_gravity_record(im, v.imu_grav + cur * 16);
  // flag hand-overs, trial point: k_imu_jac behind this kernel needs the main stream's trial poses.  One thread of this kernel
  // waits for their flag before the kernel ends -- the kernel boundary then orders k_imu_jac behind it like any other kernel,
  // without a waiting kernel of its own (5 us on this stream's queue, which is the critical one at the end of a small pass)
  if (trial && v.block_wait > 0 && blockIdx.x == 0 && threadIdx.x == 0) spin_until_flag<false>(v, 2, v.block_wait);
}

}  // namespace vc
