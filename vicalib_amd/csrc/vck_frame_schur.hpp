// vck_frame_schur.hpp -- k_frame_schur, k_part_sum: the elimination of the per-frame pose blocks (vision-only passes).
//  k_frame_schur  one wavefront per frame: H_pp, g_p from the tile Gram blocks, damping, 6x6 Cholesky, Y = L^-1 W per tile (lanes = columns);
//                 per chunk sum Y^T Y, sum Y^T z on the matrix pipe
//  k_part_sum     fixed-order sum of the chunk partials, spread over many CUs
// Kernel fragment: defines __global__ symbols, so it belongs to exactly ONE translation unit -- vc_kernels.hip, which includes the
// fragments in stage order.  Not one of the VC_HD arithmetic headers (vc_math.hpp, ..): host harnesses cannot include it.
#pragma once
#include <hip/hip_runtime.h>
#include "vc_math.hpp"
#include "vc_device.h"
#include "vc_kutil.hpp"

namespace vc {

// (defined with the step decision, vck_decide.hpp, which comes later in the translation unit: declared here for k_frame_schur's merged passes)
__device__ void merged_control(const DevView& v, Ctrl* out, double* red, bool writer);

// ------------------------------------------------------------------------------------------ frame elimination
// k_frame_schur: one workgroup per chunk of frames, one wavefront per frame (groups of 4 frames).
//  per frame   lanes 0..35 own the entries of H_pp, 36..41 those of g_p; every lane then factors the damped
//              6x6 block redundantly (wave-uniform); lanes own (tile, column) pairs of Y = L^-1 W.
//  per group   the 4 x 6 rows [Y_f | z_f] (dense over the shared columns) sit in LDS and their Gram matrix
//              sum Y^T Y, sum Y^T z is accumulated on the matrix pipe (v_mfma_f64_16x16x4_f64), 16x16
//              column-tile pairs distributed over the 4 wavefronts.
//  per chunk   part = [ sum Y^T Y (D x D, upper) | sum Y^T z (D) | per-camera sum of G (C x 256) ]
constexpr int kPrepPad = 48;
constexpr int kMaxPairsPerWave = 9;      // 8 column tiles -> 36 pairs over 4 waves
__device__ __forceinline__ int schur_ld(int D) { const int Dp = ((D + 1 + 15) / 16) * 16; return (Dp % 32 == 0) ? Dp + 16 : Dp; }

template <int MAXC, int MAXP, int MINW>
__global__ __launch_bounds__(256, MINW) void k_frame_schur(DevView v) {
  extern __shared__ __attribute__((aligned(16))) double sh[];
  __shared__ Ctrl s_ctrl;
  __shared__ CamDesc s_cd[kMaxCams];     // LDS copy of the kernel-argument table (dynamically indexed below)
  __shared__ unsigned short s_pair[4 * kMaxPairsPerWave];      // column-tile pair p -> I | J << 8
  if (threadIdx.x < kMaxCams) s_cd[threadIdx.x] = v.cd[threadIdx.x];
  {
    const int nT_ = (v.D + 1 + 15) / 16, nP_ = nT_ * (nT_ + 1) / 2;
    if ((int)threadIdx.x < nP_ && threadIdx.x < 4 * kMaxPairsPerWave) {
      int I = 0, J = 0;
      for (int k = 0; k < (int)threadIdx.x; ++k) if (++J == nT_) { ++I; J = I; }
      s_pair[threadIdx.x] = (unsigned short)(I | (J << 8));
    }
  }
  const Ctrl* ct = v.ctrl;
  if (v.merged) { merged_control(v, &s_ctrl, sh, blockIdx.x == 0); ct = &s_ctrl; }
  else __syncthreads();
  if (ct->done) return;
  const int tid = threadIdx.x, wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63;
  const int C = v.n_cams, D = v.D;
  const int nT = (D + 1 + 15) / 16, ld = schur_ld(D), nPairs = min(nT * (nT + 1) / 2, 4 * kMaxPairsPerWave);
  double* Gw = sh + wave * (C * kGStride + kPrepPad);
  double* Hs = Gw + C * kGStride;
  double* R = sh + 4 * (C * kGStride + kPrepPad);
  const int cur = ct->cur;
  const int init_scale = ct->init_scale, reuse = ct->reuse_diag;
  const double radius = ct->radius;
  const double* cams = v.cams[cur];
  const int chunk = blockIdx.x;
  const int f0 = chunk * v.chunk_frames, f1 = min(f0 + v.chunk_frames, v.n_frames);
  v4d acc[MAXP];
#pragma unroll
  for (int i = 0; i < MAXP; ++i) acc[i] = (v4d){0.0, 0.0, 0.0, 0.0};
  double gsum[MAXC][5];      // [4]: the record's side vector (lanes < 16)
#pragma unroll
  for (int c = 0; c < MAXC; ++c)
#pragma unroll
    for (int q = 0; q < 5; ++q) gsum[c][q] = 0.0;
  double csum = 0.0;      // lane t: cost of tile t of this wave's frames (the chunk's cost rides in the partials)
  double x2_noobs = 0.0;  // lane 0: parameter norm of this wave's frames that have no observations

  for (int fg = f0; fg < f1; fg += 4) {
    const int f = fg + wave;
    for (int i = lane; i < 6 * ld; i += 64) R[(wave * 6) * ld + i] = 0.0;
    const int t0 = (f < f1) ? v.frame_tile_off[f] : 0;
    const int nt = (f < f1) ? v.frame_tile_off[f + 1] - t0 : 0;
    if (lane < nt) csum += v.tile_costb[cur][t0 + lane];
    // requested once per frame, ahead of their use: the camera of every tile (lane t) and the frame's damping inputs
    const int my_cam = (lane < nt) ? v.tile_cam[t0 + lane] : 0;
    double pre_sc2[6], pre_dg[6];
#pragma unroll
    for (int i = 0; i < 6; ++i) {
      pre_sc2[i] = (nt > 0 && !init_scale) ? v.fscale2[(size_t)f * 6 + i] : 1.0;
      pre_dg[i] = (nt > 0 && reuse) ? v.fdiag[(size_t)f * 6 + i] : 1.0;
    }
    if (f < f1 && nt == 0 && lane == 0) {     // frame without observations: nothing to eliminate, keeps its pose
      const double* p = v.poses[cur] + (size_t)f * kPoseStride;
      double x2 = 0;
      for (int i = 0; i < 7; ++i) x2 += p[i] * p[i];
      double* o = v.fpart + (size_t)f * kNumScal;
      for (int i = 0; i < kNumScal; ++i) o[i] = 0.0;
      o[kScX2] = x2;
      x2_noobs += x2;
    }
    if (nt > 0) {
      for (int t = 0; t < nt; ++t) {           // full 16x16 Gram block of every tile of the frame
        double val[5];
#pragma unroll
        for (int q = 0; q < 4; ++q) { const int e = q * 64 + lane; val[q] = v.Gb[cur][(size_t)(t0 + t) * kGPack + g_pack_idx(e >> 4, e & 15)]; }      // (packed record: expanded on load)
        val[4] = (lane < 16) ? v.Gb[cur][(size_t)(t0 + t) * kGPack + kGPackGrad + lane] : 0.0;
#pragma unroll
        for (int q = 0; q < 4; ++q) Gw[t * kGStride + q * 64 + lane] = val[q];
        if (lane < 16) Gw[t * kGStride + kGGrad + lane] = val[4];
        const int c = __builtin_amdgcn_readlane(my_cam, t);      // wave-uniform: scalar branch, one camera's accumulators touched
#pragma unroll
        for (int k = 0; k < MAXC; ++k)
          if (k == c) {
#pragma unroll
            for (int q = 0; q < 5; ++q) gsum[k][q] += val[q];
          }
      }
      wave_lds_sync();
      double hval = 0.0;
      if (lane < 42) {
        for (int t = 0; t < nt; ++t) {
          const int c = __builtin_amdgcn_readlane(my_cam, t);
          double Rm[9];
          quat_to_R(cams + (size_t)c * kCamStride, Rm);
          const double* g = Gw + t * kGStride;
          if (lane < 36) {
            const int i = lane / 6, j = lane % 6, a = i / 3, ii = i % 3, b = j / 3, jj = j % 3;
            double s = 0.0;
#pragma unroll
            for (int p = 0; p < 3; ++p)
#pragma unroll
              for (int q = 0; q < 3; ++q) s += Rm[3 * p + ii] * g[(3 * a + p) * 16 + 3 * b + q] * Rm[3 * q + jj];
            hval += (a == b) ? s : -s;
          } else {
            const int i = lane - 36, a = i / 3, ii = i % 3;
            const int nk = model_nk(s_cd[c].model);
            double s = 0.0;
#pragma unroll
            for (int p = 0; p < 3; ++p) s += Rm[3 * p + ii] * gram_grad(g, 3 * a + p, nk);
            hval += (a == 0) ? -s : s;
          }
        }
        Hs[lane] = hval;
      }
      wave_lds_sync();
      double H[36], g6[6], lam[6];
#pragma unroll
      for (int i = 0; i < 36; ++i) H[i] = Hs[i];
#pragma unroll
      for (int i = 0; i < 6; ++i) g6[i] = Hs[36 + i];
#pragma unroll
      for (int i = 0; i < 6; ++i) {
        const double hd = H[i * 6 + i];
        double sc2, dg;
        if (init_scale) { sc2 = jacobi_scale2(hd); if (lane == 0) v.fscale2[(size_t)f * 6 + i] = sc2; }
        else sc2 = pre_sc2[i];
        if (!reuse) { dg = lm_clamped_diag(hd, sc2); if (lane == 0) v.fdiag[(size_t)f * 6 + i] = dg; }
        else dg = pre_dg[i];
        lam[i] = dg / (radius * sc2);
        H[i * 6 + i] = hd + lam[i];
      }
      double dinv[6];
      if (!chol_small<6>(H, dinv)) {
        if (lane == 0) atomicAdd(&v.flags[4 + 2 * v.par], 1);
#pragma unroll
        for (int i = 0; i < 36; ++i) H[i] = (i % 7 == 0) ? 1.0 : 0.0;
#pragma unroll
        for (int i = 0; i < 6; ++i) dinv[i] = 1.0;
      }
      double z[6];
#pragma unroll
      for (int i = 0; i < 6; ++i) z[i] = g6[i];
      fwd_solve_inv<6>(H, dinv, z);
      if (lane == 0) {
        double* fr = v.fr + (size_t)f * kFrStride;
        int k = 0;
#pragma unroll
        for (int i = 0; i < 6; ++i)
#pragma unroll
          for (int j = 0; j <= i; ++j) fr[kFrL + k++] = H[i * 6 + j];
#pragma unroll
        for (int i = 0; i < 6; ++i) { fr[kFrZ + i] = z[i]; fr[kFrG + i] = g6[i]; fr[kFrLam + i] = lam[i]; fr[kFrDinv + i] = dinv[i]; R[(wave * 6 + i) * ld + D] = z[i]; }
      }
      for (int idx = lane; idx < nt * 16; idx += 64) {      // Y columns: lane -> (tile, column)
        const int t = idx >> 4, j = idx & 15;
        const int c = __shfl(my_cam, t, 64);
        const int flags = s_cd[c].flags, nk = model_nk(s_cd[c].model);
        const int nrot = (flags & kCamRotFree) ? 3 : 0, ntr = (flags & kCamTransFree) ? 3 : 0;
        const int nc = nrot + ntr + ((flags & kCamKFree) ? nk : 0);
        double w[6] = {0, 0, 0, 0, 0, 0};
        if (j < nc) {
          double Rm[9];
          quat_to_R(cams + (size_t)c * kCamStride, Rm);
          const double* g = Gw + t * kGStride;
          double u[6];   // column of [Gaa Ea | GaB]
          if (j < nrot) {
#pragma unroll
            for (int r = 0; r < 6; ++r) u[r] = -(g[r * 16 + 3] * Rm[j] + g[r * 16 + 4] * Rm[3 + j] + g[r * 16 + 5] * Rm[6 + j]);
          } else {
            const int jj = (j < nrot + ntr) ? j - nrot : 6 + (j - nrot - ntr);
#pragma unroll
            for (int r = 0; r < 6; ++r) u[r] = g[r * 16 + jj];
          }
#pragma unroll
          for (int i = 0; i < 3; ++i) {   // w = Qa^T u, Qa = diag(-R, R)
            w[i] = -(Rm[i] * u[0] + Rm[3 + i] * u[1] + Rm[6 + i] * u[2]);
            w[3 + i] = Rm[i] * u[3] + Rm[3 + i] * u[4] + Rm[6 + i] * u[5];
          }
          fwd_solve_inv<6>(H, dinv, w);
          const int col = s_cd[c].col0 + j;
#pragma unroll
          for (int r = 0; r < 6; ++r) R[(wave * 6 + r) * ld + col] = w[r];
        }
        double* Yt = v.Y + (size_t)(t0 + t) * kYStride;
#pragma unroll
        for (int r = 0; r < 6; ++r) Yt[r * kUCols + j] = w[r];
      }
    }
    __syncthreads();
    {
      // accumulator q of wavefront w belongs to pair 4 q + w (compile-time index: no select chains, and the MAXP chains of
      // dependent MFMAs advance side by side); past the last pair the last one is recomputed and never written
      const double* rq = R + (lane >> 4) * ld + (lane & 15);
      int oa[MAXP], ob[MAXP];
#pragma unroll
      for (int q = 0; q < MAXP; ++q) {
        const int ij = s_pair[min(4 * q + wave, nPairs - 1)];
        oa[q] = (ij & 255) * 16; ob[q] = (ij >> 8) * 16;
      }
#pragma unroll
      for (int ks = 0; ks < 6; ++ks)
#pragma unroll
        for (int q = 0; q < MAXP; ++q) acc[q] = __builtin_amdgcn_mfma_f64_16x16x4f64(rq[ks * 4 * ld + oa[q]], rq[ks * 4 * ld + ob[q]], acc[q], 0, 0, 0);
    }
    __syncthreads();
  }
  double* part = v.part + (size_t)chunk * v.part_stride;
#pragma unroll
  for (int q = 0; q < MAXP; ++q) {
    const int p = 4 * q + wave;
    if (p < nPairs) {
      const int ij = s_pair[p], I = ij & 255, J = ij >> 8;
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const int row = I * 16 + (lane >> 4) + 4 * g, col = J * 16 + (lane & 15);
        if (row < D) { if (col < D) part[row * D + col] = acc[q][g]; else if (col == D) part[D * D + row] = acc[q][g]; }
      }
    }
  }
  // per-camera sum of G over the chunk: combine the 4 wavefronts through LDS (fixed order)
  __syncthreads();
#pragma unroll
  for (int c = 0; c < MAXC; ++c)
    if (c < C) {
#pragma unroll
      for (int q = 0; q < 4; ++q) sh[wave * (C * kGStride) + c * kGStride + q * 64 + lane] = gsum[c][q];
      if (lane < 16) sh[wave * (C * kGStride) + c * kGStride + kGGrad + lane] = gsum[c][4];
    }
  __syncthreads();
  for (int e = tid; e < C * kGStride; e += 256)
    part[D * D + D + e] = (sh[e] + sh[C * kGStride + e]) + (sh[2 * C * kGStride + e] + sh[3 * C * kGStride + e]);
  // chunk cost (sum of the tiles' robustified costs at the linearisation point), last slot of the partial record
  __syncthreads();
  csum = wave_sum(csum);
  if (lane == 0) { sh[wave] = csum; sh[4 + wave] = x2_noobs; }
  __syncthreads();
  if (tid == 0) { part[v.part_stride - 1] = (sh[0] + sh[1]) + (sh[2] + sh[3]); part[v.part_stride - 2] = (sh[4] + sh[5]) + (sh[6] + sh[7]); }
}

// Fixed-order sum of the chunk partials, spread over many CUs (one CU can only pull ~20-50 GB/s): workgroup x owns 16 entries
// (one 128-byte line per chunk); thread (entry = tid & 15, slice = tid >> 4) sums the partials k = slice (mod 32) -- all of a
// thread's loads are independent, two or three rounds of 16 --, the 32 slices are then added in order.  The result goes where its
// consumer wants it: -sum into Sbuf's S (both triangles: the producers only fill tile pairs I <= J, whose mirror image is written
// here -- entries of the lower block triangle are neither summed nor read) and g_red, the per-camera Gram sums / IMU parameter
// block / chunk scalars into part_total.  k_reduced (one workgroup) used to add slab totals, negate and mirror itself: 0.5 MB
// through one CU plus a D^2 loop of dependent round trips, 24 + 8 us at D = 67.  (A two-level version whose last workgroup per
// column added the slab totals behind a device-scope fence was 14x slower: every release fence writes the L2 back.)
constexpr int kSumEntries = 16, kSumSlices = 32;
template <int SLICES>
__device__ __forceinline__ void part_sum_block(const DevView& v, int block, double* sl /* 16 x SLICES */) {
  // (the control record is requested here and looked at once the partials have been requested as well: a finished solve costs a few
  //  wasted loads, a running one saves the record's round trip ahead of the sum's)
  const int done = v.ctrl->done;
  const int tid = threadIdx.x, e = block * kSumEntries + (tid & (kSumEntries - 1)), ks = tid / kSumEntries;
  const int stride = v.part_stride, D = v.D, DD = D * D, n = v.n_part;
  int i = 0, j = 0;
  bool live = e < stride;
  if (e < DD) { i = e / D; j = e - i * D; live = (i >> 4) <= (j >> 4); }
  double s = 0.0;
  if (live) {
    const double* src = v.part + e;
#pragma unroll 16
    for (int k = ks; k < n; k += SLICES) s += src[(size_t)k * stride];
  }
  if (done) return;
  sl[tid] = s;
  __syncthreads();
  if (tid < kSumEntries && live) {
    double t = sl[tid];
#pragma unroll
    for (int q = 1; q < SLICES; ++q) t += sl[q * kSumEntries + tid];
    double* S = v.Sbuf;
    if (e < DD) { S[e] = -t; if ((i >> 4) < (j >> 4)) S[j * D + i] = -t; }
    else if (e < DD + D) S[e] = -t;        // g_red follows S
    else v.part_total[e] = t;
  }
}
__global__ __launch_bounds__(kSumEntries * kSumSlices) void k_part_sum(DevView v) {
  __shared__ double sl[kSumEntries * kSumSlices];
  part_sum_block<kSumSlices>(v, (int)blockIdx.x, sl);
}

}  // namespace vc
