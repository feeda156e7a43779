// vci_lanes.hpp -- lane helpers of the IMU kernels (k_imu_block, k_imu_weights): DPP row operations on doubles, scans of deltas and maps over
// the lanes of a row, the two-sided sample look-up, the IMU buffers' view.  __forceinline__ functions only.
// Fragment of vc_imu_kernels.hip, included there in stage order.
#pragma once
#include <hip/hip_runtime.h>
#include "vc_math.hpp"
#include "vc_imu.hpp"
#include "vc_imu_weights.hpp"
#include "vc_device.h"

namespace vc {

// DPP row operations on doubles (two 32-bit moves).  row_shr:n -- lane i of a row reads lane i - n; row_shl:n -- lane i + n;
// lanes without a source keep `old`.
template <int CTRL> __device__ __forceinline__ double dpp_f64(double old, double x) {
  const int lo = __builtin_amdgcn_update_dpp(__double2loint(old), __double2loint(x), CTRL, 0xf, 0xf, false);
  const int hi = __builtin_amdgcn_update_dpp(__double2hiint(old), __double2hiint(x), CTRL, 0xf, 0xf, false);
  return __hiloint2double(hi, lo);
}
template <int N> __device__ __forceinline__ double row_shr(double old, double x) { return dpp_f64<0x110 + N>(old, x); }
template <int N> __device__ __forceinline__ double row_shl(double old, double x) { return dpp_f64<0x100 + N>(old, x); }
// row permutation of a double (every lane has a source: no `old` operand, no copy)
template <int CTRL> __device__ __forceinline__ double dpp_perm(double x) {
  const int lo = __builtin_amdgcn_mov_dpp(__double2loint(x), CTRL, 0xf, 0xf, false);
  const int hi = __builtin_amdgcn_mov_dpp(__double2hiint(x), CTRL, 0xf, 0xf, false);
  return __hiloint2double(hi, lo);
}
// sums over the 16 lanes of a row of N values at once, the same bits in every lane (each level adds the partner's value to the
// lane's own: commutative).  Level by level over all values: the N exchanges of a level are independent instructions.
template <int CTRL, int N> __device__ __forceinline__ void row_add_level(double* x) {
  double y[N];
#pragma unroll
  for (int e = 0; e < N; ++e) y[e] = dpp_perm<CTRL>(x[e]);
#pragma unroll
  for (int e = 0; e < N; ++e) x[e] += y[e];
}
template <int N> __device__ __forceinline__ void row_allsum_n(double* x) {
  row_add_level<0xB1, N>(x);                     // quad_perm [1 0 3 2]
  row_add_level<0x4E, N>(x);                     // quad_perm [2 3 0 1]
  row_add_level<0x141, N>(x);                    // row_half_mirror
  row_add_level<0x140, N>(x);                    // row_mirror
}
__device__ __forceinline__ double shfl16(double x, int src) { return __shfl(x, src, 16); }
__device__ __forceinline__ void delta_identity(DeltaAcc<double>* a) {
#pragma unroll
  for (int k = 0; k < 3; ++k) { a->q[k] = 0.0; a->p[k] = 0.0; a->v[k] = 0.0; }
  a->q[3] = 1.0; a->t = 0.0;
}
// a <- a followed by x
__device__ __forceinline__ void delta_then(DeltaAcc<double>* a, const DeltaAcc<double>& x) {
  PoseV<double> d;
#pragma unroll
  for (int k = 0; k < 4; ++k) d.q[k] = x.q[k];
#pragma unroll
  for (int k = 0; k < 3; ++k) { d.p[k] = x.p[k]; d.v[k] = x.v[k]; }
  imu_delta_append(a, d, x.t);
}
// one level of the inclusive scan: lanes >= N of the row take (lane - N's value) followed by their own
template <int N> __device__ __forceinline__ void delta_scan_level(DeltaAcc<double>* X, int c) {
  DeltaAcc<double> A;
#pragma unroll
  for (int k = 0; k < 4; ++k) A.q[k] = row_shr<N>(X->q[k], X->q[k]);
#pragma unroll
  for (int k = 0; k < 3; ++k) { A.p[k] = row_shr<N>(X->p[k], X->p[k]); A.v[k] = row_shr<N>(X->v[k], X->v[k]); }
  A.t = row_shr<N>(X->t, X->t);
  delta_then(&A, *X);
  if (c >= N) *X = A;
}
// one level of the suffix scan of the maps: (lane + N's map) applied after the lane's own; the last N lanes of the row receive
// the identity, whose product with their own map is that map bit for bit
template <int N> __device__ __forceinline__ void map_scan_level(double* S) {
  double B[kWMapF], O[kWMapF];
  w_map_identity(B);
#pragma unroll
  for (int e = 0; e < kWMapF; ++e) B[e] = row_shl<N>(B[e], S[e]);
  w_map_compose(B, S, O);
#pragma unroll
  for (int e = 0; e < kWMapF; ++e) S[e] = O[e];
}

// imu_range (vc_imu.hpp) with its two look-ups side by side: even lanes find the element of t0, odd lanes that of t1 -- the same
// dependent loads, once instead of twice in a row -- and neighbours swap results.  All lanes of the wavefront must be active.
__device__ __forceinline__ ImuRange imu_range_lanes(const ImuView& b, double t0, double t1, double off, int lane) {
  ImuRange r; r.valid = 0; r.k0 = 0; r.k1 = -1; r.i0 = r.i1 = 0; r.first_end = r.last_end = 0;
  if (b.n < 2) return r;
  const bool odd = lane & 1;
  int idx, endc, le;
  imu_element_index(b, odd ? t1 : t0, off, &idx, &endc, &le);
  const int idx_o = __shfl_xor(idx, 1, 64), endc_o = __shfl_xor(endc, 1, 64), le_o = __shfl_xor(le, 1, 64);
  r.valid = (t0 >= b.t[0] + off && t0 <= b.t[b.n - 1] + off) ? 1 : 0;      // HasElement :122-125
  r.i0 = odd ? idx_o : idx; r.first_end = odd ? endc_o : endc;
  r.i1 = odd ? idx : idx_o; r.last_end = odd ? endc : endc_o;
  r.k0 = r.i0 + 1;
  r.k1 = odd ? le : le_o;
  if (r.k1 < r.i0) r.k1 = r.i0;
  return r;
}

__device__ __forceinline__ ImuView imu_view(const DevView& v) { ImuView b = {v.imu_t, v.imu_w, v.imu_a, v.n_imu, v.imu_avg_dt}; return b; }

}  // namespace vc
