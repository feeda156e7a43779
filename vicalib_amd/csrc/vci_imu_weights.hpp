// vci_imu_weights.hpp -- k_imu_weights: 16 lanes per block: UpdateImuWeights (vicalibrator.h:723-799) interval-parallel (vc_imu_weights.hpp).
// Kernel fragment of vc_imu_kernels.hip alone (defines __global__ symbols; included there in stage order; not for host harnesses).
#pragma once
#include <hip/hip_runtime.h>
#include "vc_math.hpp"
#include "vc_imu.hpp"
#include "vc_imu_weights.hpp"
#include "vc_device.h"
#include "vc_kutil.hpp"
#include "vci_lanes.hpp"

namespace vc {

// UpdateImuWeights from the accepted state (vicalibrator.h:723-799), interval-parallel (vc_imu_weights.hpp, second half).
// 16 lanes per IMU block, four blocks per wavefront, one wavefront per workgroup.  A round handles 16 sample intervals of every
// block (cfg3: 12 per block, one round), lane i = interval i:
//   1. the interval's RK4 delta from the identity state (values only, vc_imu.hpp);
//   2. inclusive scan of the deltas over the 16 lanes (composition is associative): lane i learns the state its interval starts
//      from, q_start * Q_prefix, without walking the block;
//   3. the interval's maps, formed ONCE -- F (41 structural entries) and Q = G R G^T (55) -- from that quaternion;
//   4. the recurrence Sigma <- F Sigma F^T + Q unrolled: Sigma_end = sum_k P_k Q_k P_k^T with P_k the product of the maps after
//      interval k.  A suffix scan over the lanes gives P_k (the block form of F is closed under products), every lane conjugates
//      its own Q, a butterfly sums the 55 entries: no step of the recurrence waits for the one before it.
// All lane exchanges are DPP row operations (rows of 16 lanes = the groups): no LDS round trip anywhere in 1-4.
// Then the projection through the residual's Jacobian in registers (every lane holds Sigma), J Sigma J^T = L L^T by nine lanes
// (lane = row, pivots and pivot columns by 16-lane shuffles) and the stored factor W = L^-T:  W W^T = (J Sigma J^T)^-1 exactly
// as for the reference's symmetric square root (vicalibrator.h:783-796), and cost, gradient and Gauss-Newton Hessian of the
// block depend on W only through W W^T -- same optimisation, no 9x9 eigen-decomposition.
constexpr int kWLds = 184;                       // per block: the factor's rows for the inverse (81) | frame poses j-1, j (16) | v_{j-1} (4) | IMU parameters (15) | Sigma (55)
constexpr int kWPose = 88, kWVel = 104, kWImu = 108, kWSig = 128;
// phase stamps of the first wavefront (profiling builds only, -DVC_W_STAMPS): 100 MHz s_memrealtime ticks in dbg[0..15]
#ifdef VC_W_STAMPS
#define WSTAMP(i) do { if (blockIdx.x == 0 && threadIdx.x == 0) v.dbg[i] = (long long)__builtin_amdgcn_s_memrealtime(); } while (0)
#else
#define WSTAMP(i) do { } while (0)
#endif
__global__ __launch_bounds__(64) void k_imu_weights(DevView v, int wr) {
  __shared__ __attribute__((aligned(16))) double w_lds[4 * kWLds];
  const Ctrl* ct = v.ctrl;
  const int lane = threadIdx.x;
  const int grp = lane >> 4, c = lane & 15;      // c: interval of the round; row of the projection afterwards
  const int n_blocks = v.n_frames - 1;
  const int s_raw = blockIdx.x * 4 + grp;
  const bool exists = s_raw < n_blocks;
  const int s = exists ? s_raw : n_blocks - 1;   // groups past the end shadow the last block and store nothing
  double* L = w_lds + grp * kWLds;
  // the buffer being written must end up complete: blocks that keep their weight (no samples, singular projection) and passes
  // queued behind a finished solve copy the current one -- at the end, off the path of the blocks that get a new weight
  // A pass that is void after a flag time-out (vc_kutil.hpp), and every pass queued behind it, must leave BOTH buffers alone: the
  // resumed pass linearises with the weights its predecessor left in wsqrtb[wr of the void pass], which is the buffer the next
  // queued pass would write (round 4: a time-out in the middle of a solve resumed with the void pass's own weights there -- same
  // state, one update too far: costs off by 1e-5 .. 5e-4 for a few iterations.  A first-pass time-out hides it: both buffers
  // hold the same numbers).  The host takes the buffer index back from its ring (resume_after_sync_timeout).
  if (v.sync_seq > 0) { const long long m = sync_marked(v); if (m != 0 && m <= v.sync_seq) return; }      // wave-uniform
  if (ct->done == kDoneSyncTimeout) return;
  if (ct->done || !v.weights_on) {               // wave-uniform
    if (exists) for (int e = c; e < 81; e += 16) v.wsqrtb[1 - wr][(size_t)s * 81 + e] = v.wsqrtb[wr][(size_t)s * 81 + e];
    return;
  }
  WSTAMP(0);
  const int j = s + 1;
  // The block's state, one value per lane: frames j - 1 and j are 16 consecutive doubles, the IMU parameters 15; both state buffers
  // are requested before the control record says which one is current (one round of loads less), the current one goes to LDS and
  // every lane reads what it needs when it needs it -- nothing of this sits in registers across the phases below.
  {
    const double p0 = v.poses[0][(size_t)(j - 1) * kPoseStride + c], p1 = v.poses[1][(size_t)(j - 1) * kPoseStride + c];
    const double u0 = v.vel[0][(size_t)(j - 1) * 4 + (c & 3)], u1 = v.vel[1][(size_t)(j - 1) * 4 + (c & 3)];
    const int ci = c < 15 ? c : 14;
    const double i0 = v.imus[0][ci], i1 = v.imus[1][ci];
    const bool one = ct->cur != 0;
    L[kWPose + c] = one ? p1 : p0;
    if (c < 4) L[kWVel + c] = one ? u1 : u0;
    if (c < 15) L[kWImu + c] = one ? i1 : i0;
  }
  const double t_start = v.frame_time[j - 1], t_end = v.frame_time[j];
  wave_lds_sync();
  double b[6], sf[6];
#pragma unroll
  for (int i = 0; i < 6; ++i) { b[i] = L[kWImu + 2 + i]; sf[i] = L[kWImu + 8 + i]; }
  const double toff = L[kWImu + 14];
  const ImuView buf = imu_view(v);
  const ImuRange rg = imu_range_lanes(buf, t_start, t_end, toff, lane);
  const bool live = exists && rg.valid;          // an empty range keeps its current weight (vicalibrator.h:731-733)
  const double sg2 = v.gyro_sigma * v.gyro_sigma, sa2 = v.accel_sigma * v.accel_sigma;
  const int n_int = live ? (rg.k1 - rg.k0 + 1) + 1 : 0;      // intervals between the n_meas = n_int + 1 range elements
  int n_max = n_int;                             // the wave runs to its longest group
#pragma unroll
  for (int o = 32; o >= 16; o >>= 1) n_max = max(n_max, __shfl_xor(n_max, o, 64));
  DeltaAcc<double> carry;                        // the block's delta up to the current round
  delta_identity(&carry);
  // Sigma (packed lower triangle) rests in LDS between the rounds and until the projection: 55 doubles that would otherwise sit
  // in registers (or, as they did, in scratch memory) across the maps of every round
  const double g0[3] = {0.0, 0.0, 0.0};
  WSTAMP(1);
#pragma unroll 1
  for (int base = 0; base < n_max; base += 16) {
    const int m = base + c + 1;                  // interval m runs from range element m - 1 to m
    Meas<double> z0, z1;
#pragma unroll
    for (int k = 0; k < 3; ++k) { z0.w[k] = z0.a[k] = z1.w[k] = z1.a[k] = 0.0; }
    z0.time = z1.time = 0.0;
    if (m <= n_int) { imu_range_get_flat(buf, rg, toff, t_start, t_end, m - 1, &z0); imu_range_get_flat(buf, rg, toff, t_start, t_end, m, &z1); }
    const bool act = z1.time != z0.time;         // a zero-length interval is skipped (types.h:150-152)
    WSTAMP(2);
    // 1. the interval's delta from the identity
    DeltaAcc<double> X;
    {
      PoseV<double> d;
#pragma unroll
      for (int k = 0; k < 3; ++k) { d.q[k] = 0.0; d.p[k] = 0.0; d.v[k] = 0.0; }
      d.q[3] = 1.0;
      imu_rk4_step(&d, z0, z1, b, sf, g0);       // (returns at once for a skipped interval: the identity)
#pragma unroll
      for (int k = 0; k < 4; ++k) X.q[k] = d.q[k];
#pragma unroll
      for (int k = 0; k < 3; ++k) { X.p[k] = d.p[k]; X.v[k] = d.v[k]; }
      X.t = z1.time - z0.time;
    }
    WSTAMP(3);
    // 2. inclusive scan over the group's 16 lanes
    delta_scan_level<1>(&X, c); delta_scan_level<2>(&X, c); delta_scan_level<4>(&X, c); delta_scan_level<8>(&X, c);
    double q_st[4];
    {
      double qe[4], ident[4] = {0.0, 0.0, 0.0, 1.0};      // everything before this lane's interval: the carry, then lanes 0 .. c - 1
#pragma unroll
      for (int k = 0; k < 4; ++k) ident[k] = row_shr<1>(ident[k], X.q[k]);
      quat_mul(carry.q, ident, qe);
      const double q1[4] = {L[kWPose + 0], L[kWPose + 1], L[kWPose + 2], L[kWPose + 3]};
      quat_mul(q1, qe, q_st);
      DeltaAcc<double> Tt;                       // the round's total (lane 15) joins the carry
#pragma unroll
      for (int k = 0; k < 4; ++k) Tt.q[k] = shfl16(X.q[k], 15);
#pragma unroll
      for (int k = 0; k < 3; ++k) { Tt.p[k] = shfl16(X.p[k], 15); Tt.v[k] = shfl16(X.v[k], 15); }
      Tt.t = shfl16(X.t, 15);
      delta_then(&carry, Tt);
    }
    WSTAMP(4);
    // 3. the interval's maps (a skipped interval: the identity map and no noise)
    double F[kWMapF], G[kWMapG];
    if (act) w_interval_maps(q_st, z0, z1, b, sf, F, G);
    else {
      w_map_identity(F);
#pragma unroll
      for (int e = 0; e < kWMapG; ++e) G[e] = 0.0;
    }
    WSTAMP(5);
    // 4. Sigma_out = S_0 Sigma_in S_0^T + sum_k P_k G_k R G_k^T P_k^T  (S_0: all maps of the round, P_k: those after interval k)
    map_scan_level<1>(F); map_scan_level<2>(F); map_scan_level<4>(F); map_scan_level<8>(F);     // F: F_15 ... F_c
    double term[kWMapQ];
    {
      double P[kWMapF];
      w_map_identity(P);
#pragma unroll
      for (int e = 0; e < kWMapF; ++e) P[e] = row_shl<1>(P[e], F[e]);        // the maps after this lane's interval
      WSTAMP(6);
      w_noise_term(P, G, sg2, sa2, term);
    }
    if (base > 0) {                              // a later round: the first lane takes Sigma_in through the whole round
      double Sp[kWMapQ], Sin[kWMapQ];
#pragma unroll
      for (int e = 0; e < kWMapQ; ++e) Sp[e] = L[kWSig + e];
      w_conj(F, Sp, Sin);
#pragma unroll
      for (int e = 0; e < kWMapQ; ++e) term[e] += (c == 0) ? Sin[e] : 0.0;
    }
    WSTAMP(7);
#pragma unroll
    for (int e0 = 0; e0 < kWMapQ; e0 += 11) row_allsum_n<11>(term + e0);
    wave_lds_sync();                             // (a later round has read the previous Sigma above)
    if (c == 0) {
#pragma unroll
      for (int e = 0; e < kWMapQ; ++e) L[kWSig + e] = term[e];
    }
    wave_lds_sync();
  }
  WSTAMP(8);
  // the predicted state from the block's delta (vc_imu.hpp), then J = dLog_dSE3(T_pred T2^-1) dt1t2_dt1(T_pred, T2^-1) with
  // the velocity identity appended (9 x 10); lane i (< 9) forms row i of P = J Sigma J^T
  double a[9];
  {
    double Sp[kWMapQ];
#pragma unroll
    for (int e = 0; e < kWMapQ; ++e) Sp[e] = (n_max > 0) ? L[kWSig + e] : 0.0;
    double T1[7], T2[7], v1[3], gw[3], q_end[4], p_end[3], rp[3];
#pragma unroll
    for (int i = 0; i < 7; ++i) { T1[i] = L[kWPose + i]; T2[i] = L[kWPose + 8 + i]; }
#pragma unroll
    for (int i = 0; i < 3; ++i) v1[i] = L[kWVel + i];
    { const double g2[2] = {L[kWImu + 0], L[kWImu + 1]}; imu_gravity(g2, gw); }
    quat_mul(T1, carry.q, q_end);
    tq_rotate(T1, carry.p, rp);
    const double ht2 = 0.5 * (carry.t * carry.t);
#pragma unroll
    for (int i = 0; i < 3; ++i) p_end[i] = ((T1[4 + i] + v1[i] * carry.t) - gw[i] * ht2) + rp[i];
    double rel[7], t2w[7], dl[42], m34[12], m44[16], Jr[6][7], mine[10];
    w_projection_prepare(q_end, p_end, T2, rel, t2w);
    w_dlog_dse3_lean(rel, dl);
    w_dqx_dq(q_end, t2w + 4, m34);
    w_dq1q2_dq1(t2w, m44);
#pragma unroll
    for (int i = 0; i < 6; ++i) w_projection_row(dl, m34, m44, i, Jr[i]);
#pragma unroll
    for (int q = 0; q < 10; ++q) {
      double x = (q >= 7 && c == q - 1) ? 1.0 : 0.0;            // rows 6..8: the velocity identity
#pragma unroll
      for (int i = 0; i < 6; ++i) x = (q < 7 && c == i) ? Jr[i][q] : x;
      mine[q] = x;
    }
    double JS[10];
#pragma unroll
    for (int q = 0; q < 10; ++q) {
      double acc = 0.0;
#pragma unroll
      for (int r = 0; r < 10; ++r) acc += mine[r] * Sp[w_qidx(r, q)];
      JS[q] = acc;
    }
#pragma unroll
    for (int jj = 0; jj < 6; ++jj) {
      double acc = 0.0;
#pragma unroll
      for (int q = 0; q < 7; ++q) acc += JS[q] * Jr[jj][q];
      a[jj] = acc;
    }
#pragma unroll
    for (int jj = 6; jj < 9; ++jj) a[jj] = JS[jj + 1];
  }
  WSTAMP(9);
  // Cholesky P = L L^T, lane i (< 9) = row i in registers: the pivot and the pivot column travel by 16-lane shuffles
  double idg[9];
  bool ok = true;
#pragma unroll
  for (int cc = 0; cc < 9; ++cc) {
    const double d = shfl16(a[cc], cc);
    ok = ok && (d > 0.0);
    const double id = (d > 0.0) ? fast_rsqrt(d) : 0.0;
    idg[cc] = id;
    const double li = a[cc] * id;                // L[i][cc] for rows i >= cc (rows above: unused)
#pragma unroll
    for (int k = cc + 1; k < 9; ++k) a[k] -= li * shfl16(li, k);
    a[cc] = li;
  }
  if (c < 9) {
#pragma unroll
    for (int k = 0; k < 9; ++k) L[c * 9 + k] = a[k];             // the factor's row c (entries k <= c)
  }
  wave_lds_sync();
  WSTAMP(10);
  if (live && !ok && c == 0) atomicAdd((unsigned long long*)&v.dbg[20], 1ull);     // singular projection: keeps the previous weight (counted)
  if (exists && !(live && ok)) for (int e = c; e < 81; e += 16) v.wsqrtb[1 - wr][(size_t)s * 81 + e] = v.wsqrtb[wr][(size_t)s * 81 + e];
  if (live && ok && c < 9) {                     // column c of X = L^-1
    double x[9];
#pragma unroll
    for (int i = 0; i < 9; ++i) x[i] = 0.0;
#pragma unroll
    for (int i = 0; i < 9; ++i) {
      double acc = (i == c) ? 1.0 : 0.0;
#pragma unroll
      for (int k = 0; k < 9; ++k) if (k < i) acc -= L[i * 9 + k] * x[k];
      x[i] = (i >= c) ? acc * idg[i] : 0.0;
    }
    double* w = v.wsqrtb[1 - wr] + (size_t)s * 81;       // W[a][b] = X[b][a]
#pragma unroll
    for (int i = 0; i < 9; ++i) w[c * 9 + i] = x[i];
  }
  WSTAMP(11);
}

}  // namespace vc
