// vck_reduced.hpp -- k_reduced: the reduced system on the shared parameters.
// One workgroup: camera blocks -> packed reduced system, damped Cholesky, delta_s, trial state of the shared parameters.
// Kernel fragment: defines __global__ symbols, so it belongs to exactly ONE translation unit -- vc_kernels.hip, which includes the
// fragments in stage order.  Not one of the VC_HD arithmetic headers (vc_math.hpp, ..): host harnesses cannot include it.
#pragma once
#include <hip/hip_runtime.h>
#include "vc_math.hpp"
#include "vc_device.h"
#include "vc_kutil.hpp"
#include "vc_shared_blocks.hpp"

namespace vc {

// (kSmallD, vc_device.h: reduced systems up to this width are solved by one wavefront; above it the workgroup-wide LDS factorisation is faster)
// Phase A of the reduced system (one workgroup):
// Sbuf = [ S = H_ss - sum Y^T Y (full symmetric, undamped) | g_red | diag(H_ss) | g_s | cost, 0 ]
struct FinalLds { double gsum[(kMaxCams + 1) * kGStride]; double P[kMaxCams * 256]; double T1[kMaxCams * 256]; double red[256]; double camq[kMaxCams * 4]; double gc[kMaxCams * 16]; };
// shader-clock stamps of k_reduced's phases (tools/dbg_stamps.py): profiling builds only (-DVC_REDUCED_STAMPS) -- each stamp is
// a global store whose acknowledgement the next barrier waits for (~1.5k cycles apiece)
#ifdef VC_REDUCED_STAMPS
// (round 6: the stamps are kept in LDS and copied out at the kernel's end -- as global stores every stamp cost ~1.5k cycles at the next barrier)
__shared__ long long s_rst[32];
#define VC_STAMP(i) do { if (threadIdx.x == 0) s_rst[i] = (long long)__builtin_readcyclecounter(); } while (0)
#else
#define VC_STAMP(i) do { } while (0)
#endif
}  // namespace vc
// (included here, not at the top: vc_reduced_tail.hpp stamps through VC_STAMP, which profiling builds define just above -- with s_rst inside vc::)
#include "vc_reduced_tail.hpp"
namespace vc {
// S: v.Sbuf, or (single process, D <= kSmallD) an LDS image of it that this phase fills first -- every read-modify-write of the
// phase and the solve's row loads then stay on chip (three L2 round trips less on the critical path); the kernel writes it back.
// top / top_rows (early Gram, DevView::gram_top_stride): the [Y | z] rows of the chain's top-level frames (LDS, 64 rows x kTopLd, zero
// beyond the rows and beyond column D) -- their Gram sums are subtracted here
constexpr int kTopLd = 34;
// the top-level frames' Gram sums (early Gram, D + 1 <= 32 columns): S -= Y^T Y, g_red -= Y^T z on the matrix pipe.  The (at most 64, zero-padded) rows are
// the k dimension, the column tiles (0,0), (0,1), (1,1) one wavefront each (v_mfma_f64_16x16x4; entries (i, j) and (j, i) are the same products in the same
// order: S stays symmetric to the bit).  (As a scalar loop -- thread per entry, two LDS reads per row and entry -- this took 6 us: 0.7 MB through the LDS pipe.)
__device__ __forceinline__ void top_gram_subtract(double* S, int D, const double* top, int top_rows) {
  const int tid = threadIdx.x;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63;
  if (wave < 3) {
    const int I = wave == 2 ? 1 : 0, J = wave == 0 ? 0 : 1;
    const double* pa = top + (lane >> 4) * kTopLd + I * 16 + (lane & 15);
    const double* pb = top + (lane >> 4) * kTopLd + J * 16 + (lane & 15);
    // (four accumulators over the 16 k-steps of the 64 padded rows: the instruction's ~300 cycles of latency four times, not sixteen)
    v4d ac[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) ac[u] = (v4d){0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int ks = 0; ks < 16; ks += 4) {
      if (4 * ks < top_rows) {      // (wave-uniform)
#pragma unroll
        for (int u = 0; u < 4; ++u) ac[u] = __builtin_amdgcn_mfma_f64_16x16x4f64(pa[(ks + u) * 4 * kTopLd], pb[(ks + u) * 4 * kTopLd], ac[u], 0, 0, 0);
      }
    }
    const v4d acc = (ac[0] + ac[1]) + (ac[2] + ac[3]);
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const int row = I * 16 + (lane >> 4) + 4 * g, col = J * 16 + (lane & 15);
      if (row < D) {
        if (col < D) { S[row * D + col] -= acc[g]; if (I != J) S[col * D + row] -= acc[g]; }
        else if (col == D) S[D * D + row] -= acc[g];
      }
    }
  }
}
// rows of the pinned frames of a sharded chain (separator of this rank, ghost of the next rank's): straight into the reduced system
__device__ __forceinline__ void pinned_rows_phase(const DevView& v, double* S, double* gred, double* hd, double* gs) {
  const int tid = threadIdx.x, D = v.D;
  for (int slot = 0; slot < 2; ++slot) {
    if (!(slot ? v.pin_last : v.pin_first)) continue;
    const int sc = slot ? v.sep_col1 : v.sep_col0;
    const double* st = v.sep_strip + (size_t)slot * 9 * v.ldw;
    for (int e = tid; e < 9 * (D + 1); e += 256) {
      const int i = e / (D + 1), col = e % (D + 1);
      const double val = st[i * v.ldw + col];
      if (col == D) { gred[sc + i] += val; gs[sc + i] += val; }
      else if (col < sc) { const double sn = S[col * D + sc + i] + val; S[col * D + sc + i] = sn; S[(sc + i) * D + col] = sn; }
      else if (col >= sc + i) {            // each pair once, both triangles written
        const double sn = S[(sc + i) * D + col] + val;
        S[(sc + i) * D + col] = sn;
        if (col == sc + i) hd[sc + i] += val; else S[col * D + sc + i] = sn;
      }
    }
    __syncthreads();
  }
}
__device__ __forceinline__ void schur_final_phase(const DevView& v, int cur, FinalLds& L, double* x2_noobs, const CamDesc* cd /* LDS copy of v.cd */, const int* ipc /* ... of v.imu_param_col */,
                                                  double* S, bool s_in_lds, const double* top = nullptr, int top_rows = 0) {
  VC_STAMP(0);
  const int tid = threadIdx.x, D = v.D, C = v.n_cams;
  if (v.hadd_early) {
    // (round 6) the camera blocks, the IMU block and the chunk costs were formed ahead of this launch (DevView::hadd, vc_shared_blocks.hpp): the
    // reduced system is Sbuf (the frames' partial sums, k_part_sum) + that record, minus the top-level frames' Gram sums
    const double* H = v.hadd;
    const int nS = D * D + D, nAll = nS + 2 * D + 2;
    if (s_in_lds) {
      constexpr int kAIter = (kSmallD * kSmallD + 3 * kSmallD + 2 + 255) / 256;
      double s_in[kAIter], h_in[kAIter];
#pragma unroll
      for (int q = 0; q < kAIter; ++q) { const int e = tid + 256 * q; s_in[q] = e < nS ? v.Sbuf[e] : 0.0; h_in[q] = e < nAll ? H[e] : 0.0; }
#pragma unroll
      for (int q = 0; q < kAIter; ++q) { const int e = tid + 256 * q; if (e < nAll) S[e] = s_in[q] + h_in[q]; }
      if (top) { __syncthreads(); top_gram_subtract(S, D, top, top_rows); }
    } else {
      // (eight entries per thread and round: all loads out before the first store -- the compiler cannot tell S and H apart, a plain loop is one
      //  memory round trip per entry: 14.7k cycles at D = 67)
      for (int e0 = tid; e0 < nAll; e0 += 8 * 256) {
        double a[8], h[8];
#pragma unroll
        for (int q = 0; q < 8; ++q) { const int e = e0 + 256 * q; a[q] = e < nS ? S[e] : 0.0; h[q] = e < nAll ? H[e] : 0.0; }
#pragma unroll
        for (int q = 0; q < 8; ++q) { const int e = e0 + 256 * q; if (e < nAll) S[e] = a[q] + h[q]; }
      }
    }
    VC_STAMP(1); VC_STAMP(2); VC_STAMP(3);
    __syncthreads();
    if (v.imu_on) pinned_rows_phase(v, S, S + D * D, S + nS, S + nS + D);
    return;
  }
  // (all of a thread's loads go out before the first is stored to LDS: a plain copy loop is one memory round trip per iteration)
  constexpr int kSIter = (kSmallD * kSmallD + kSmallD + 255) / 256;
  double s_in[kSIter];
  if (s_in_lds) {      // S and g_red as k_part_sum left them
#pragma unroll
    for (int q = 0; q < kSIter; ++q) { const int e = tid + 256 * q; s_in[q] = e < D * D + D ? v.Sbuf[e] : 0.0; }
  }
  double* gred = S + D * D;
  double* hd = gred + D;
  double* gs = hd + D;
  double* sc = gs + D;
  const int stride = v.part_stride;
  // S = -sum of the partials (both triangles) and g_red are in place (k_part_sum's last workgroups); the rest of the summed
  // record -- per-camera Gram sums, IMU parameter block, chunk scalars -- comes from part_total
  const double* ptot = v.part_total;
  // camera rotations: fetched now, under the loads' latency, instead of one dependent global load per camera later
  if (tid < C * 4) L.camq[tid] = v.cams[cur][(size_t)(tid >> 2) * kCamStride + (tid & 3)];
  for (int e0 = D * D + D + tid; e0 < stride - 1; e0 += 4 * 256) {
    double t[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) { const int e = e0 + 256 * q; t[q] = e < stride - 1 ? ptot[e] : 0.0; }
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int e = e0 + 256 * q;
      if (e < stride - 2) L.gsum[e - D * D - D] = t[q];
      else if (e == stride - 2) *x2_noobs = t[q];                 // x2 of observation-less frames
    }
  }
  if (s_in_lds) {
#pragma unroll
    for (int q = 0; q < kSIter; ++q) { const int e = tid + 256 * q; if (e < D * D + D) S[e] = s_in[q]; }
    if (top) { __syncthreads(); top_gram_subtract(S, D, top, top_rows); }
  }
  VC_STAMP(1);
  for (int i = tid; i < D; i += 256) { hd[i] = 0.0; gs[i] = 0.0; }
  if (tid == 0) { sc[0] = 0.5 * ptot[stride - 1]; sc[1] = 0.0; }      // chunk costs (the chain path's k_chain_init fills the same slot)
  __syncthreads();
  VC_STAMP(2);
  shared_blocks_phase(v, 256, L.gsum, L.P, L.camq, cd, ipc, S, gred, hd, gs);
  VC_STAMP(3);
  if (v.imu_on) pinned_rows_phase(v, S, gred, hd, gs);
}

// ------------------------------------------------------------------------------------------ reduced solve
// Phase B.  Damped Cholesky of the augmented matrix [S + Lambda, g; g^T, .] (the forward substitution
// rides along as the extra row), back substitution, then the trial state of the shared parameters
// (cams[1-cur] <- Plus(cams[cur], delta_s)) and their scalar terms scal[8..15].
//   D <= 32: one wavefront, rows in registers, pivots exchanged with v_readlane (no barriers);
//   D  > 32: workgroup-wide in LDS.
// Lane i keeps row i of the augmented matrix in registers (static indices: all loops over columns are
// unrolled to DMAX), pivots and pivot columns travel through v_readlane; the factor goes to LDS (Lt: DMAX x ldt) for the
// back-substitution only.  x: D.
// (the arguments by value: a function that is not inlined and takes the DevView by reference makes its caller keep a copy of the
//  whole record in scratch memory -- 1 KB per lane and a slower launch)
struct SmallSolveArgs { int D; double* sscale2; double* sdiag; double* slam; int* bad_flag; long long* dbg; };
#ifndef VC_SMALL_SOLVE_BCAST
#define VC_SMALL_SOLVE_BCAST 1      // (0: pivot columns through v_readlane, the form of rounds 2-5 -- A/B builds)
#endif
template <int DMAX>
__device__ __forceinline__ void solve_small_wave(const SmallSolveArgs v, const Ctrl* ct, int lane, double* Lt, double* x, double pre_sc2, double pre_dg, const double* S /* v.Sbuf or its LDS image */,
                                                 double* bc /* LDS, 2 x 64: the pivot column's broadcast image */) {
  const int D = v.D;
  constexpr int ldt = DMAX + 2;
  const double* gred = S + D * D;
  const double* hd = gred + D;
#ifdef VC_REDUCED_STAMPS
  if (lane == 0) s_rst[8] = (long long)__builtin_readcyclecounter();
#endif
  double row[DMAX];
  {
    // one base address per lane (row `lane` of S; g_red for lane D and, harmlessly, beyond), the column as an immediate offset
    const double* rp = lane < D ? S + lane * D : gred;
#pragma unroll
    for (int k = 0; k < DMAX; ++k) { double t = 0.0; if (k < D) t = rp[k]; row[k] = lane <= D ? t : 0.0; }
  }
#if VC_SMALL_SOLVE_BCAST
  double diag = lane < D ? S[lane * D + lane] : 0.0;      // row `lane`'s diagonal entry, kept apart (see the factorisation below)
#endif
  double lam = 0.0;
  if (lane < D) {
    double sc2, dg;
    // pre_sc2 / pre_dg: v.sscale2[lane] / v.sdiag[lane], requested at kernel entry (only read when they are valid)
    if (ct->init_scale) { sc2 = jacobi_scale2(hd[lane]); v.sscale2[lane] = sc2; } else sc2 = pre_sc2;
    if (!ct->reuse_diag) { dg = lm_clamped_diag(hd[lane], sc2); v.sdiag[lane] = dg; } else dg = pre_dg;
    lam = dg / (ct->radius * sc2);
    v.slam[lane] = lam;
    // the tail's inputs ride along in LDS behind x: damping and g_s of this column
    x[kSmallD + 1 + lane] = lam;
    x[2 * (kSmallD + 1) + lane] = hd[D + lane];
  }
#pragma unroll
  for (int k = 0; k < DMAX; ++k) row[k] += (k == lane) ? lam : 0.0;
#if VC_SMALL_SOLVE_BCAST
  diag += lam;
#endif
#ifdef VC_REDUCED_STAMPS
#define VC_SS(i) do { __builtin_amdgcn_s_waitcnt(0); __builtin_amdgcn_sched_barrier(0); if (lane == 0) s_rst[8 + (i)] = (long long)__builtin_readcyclecounter(); __builtin_amdgcn_sched_barrier(0); } while (0)
#else
#define VC_SS(i) do { } while (0)
#endif
  VC_SS(1);
  // Every loop below is fully unrolled (j, k compile-time): register indices are static, pivots and pivot columns travel
  // as scalars through v_readlane -- no LDS round trip and no select chains inside the dependent chain.  The column loop
  // has no branch and no store (one scheduling region): the trailing updates of column j fill the latency of column
  // j + 1's reciprocal square root.  Columns >= D only ever hold zeros (or, for column D, unused values): their steps run
  // on harmless operands (pivot forced to 1) and are not checked, so the loop needs no bound on j or k.
  bool bad = false;
#if VC_SMALL_SOLVE_BCAST
  // Round 6.  What a pivot costs is its DEPENDENT chain, and on a lone wavefront every link is ~10 cycles (a trip through LDS ~130): the
  // v_readlane form paid 2 v_readlane + SGPR hazard + FMA per entry of the trailing update (~460 cycles per pivot at D = 29), and a first
  // LDS-broadcast form put the LDS round trip of column j + 1 between pivot j and pivot j + 1 (~350).  Now:
  //   * the DIAGONAL entry of row i lives in a register of its own (`diag`): it only ever needs the lane's own l_ij, so the next pivot is
  //     one FMA and one v_readlane behind l_ij, and its reciprocal square root (v_rsq_f64 + two Newton steps; the pivot's sign is tested
  //     beside it, not ahead of it) starts at once;
  //   * column j + 1 -- the only one pivot j + 1 waits for -- takes l_(j+1)j through v_readlane;
  //   * every other column takes the pivot column from an LDS broadcast image (one ds_write_b64 per lane, two entries per wave-uniform read)
  //     and applies it ONE PIVOT LATE, behind the next pivot's chain: the LDS latency is never waited for.
  // A row's updates arrive in another order than in the v_readlane form (column j + 1: pivot j ahead of pivot j - 1); no lane select for the
  // pivot's own row: row j's entry j is the pivot itself (same FMAs as `diag`).
  double ipiv;
  {
    const double d0 = readlane_f64(diag, 0);
    const bool ok = d0 > 0.0;
    bad |= (0 < D) & !ok;
    const double y = fast_rsqrt(d0);
    ipiv = ok ? y : 1.0;
  }
  double lprev = 0.0, bprev[DMAX];
#pragma unroll
  for (int k = 0; k < DMAX; ++k) bprev[k] = 0.0;
#pragma unroll
  for (int j = 0; j < DMAX; ++j) {
    const double lij = row[j] * ipiv;
    row[j] = lij * ipiv;      // what the back-substitution wants: column j of L over its diagonal entry (off the dependent chain)
    if (j + 1 < DMAX) {
      diag -= lij * lij;
      const double dn = readlane_f64(diag, j + 1);
      double bnew[DMAX];
      if (j + 2 < DMAX) {
        double* col = bc + (j & 1) * 64;
        col[lane] = lij;
        wave_lds_sync_local();
#pragma unroll
        for (int k = j + 2; k < DMAX; ++k) bnew[k] = col[k];
      }
      __builtin_amdgcn_sched_barrier(0);      // (the reads are ISSUED here -- the scheduler otherwise sinks them, and the store, to their uses one pivot later)
      const bool ok = dn > 0.0;
      bad |= (j + 1 < D) & !ok;
      const double y = fast_rsqrt(dn);      // (of a pivot <= 0: inf / NaN, dropped by the select)
      const double ipn = ok ? y : 1.0;
      row[j + 1] -= lij * readlane_f64(lij, j + 1);
      // pivot j - 1's column, read one pivot ago: columns j + 1 ..
#pragma unroll
      for (int k = j + 1; k < DMAX; ++k) row[k] -= lprev * bprev[k];
      lprev = lij;
#pragma unroll
      for (int k = j + 2; k < DMAX; ++k) bprev[k] = bnew[k];
      ipiv = ipn;
    }
  }
#else
#pragma unroll
  for (int j = 0; j < DMAX; ++j) {
    const double mine = row[j];
    double d = readlane_f64(mine, j);
    const bool ok = d > 0.0;
    bad |= (j < D) & !ok;
    d = ok ? d : 1.0;
    const double ipiv = fast_rsqrt(d);
    const double lij = (lane == j) ? d * ipiv : mine * ipiv;
    row[j] = lij * ipiv;      // what the back-substitution wants: column j of L over its diagonal entry (off the dependent chain)
#pragma unroll
    for (int k = j + 1; k < DMAX; ++k) row[k] -= lij * readlane_f64(lij, k);
  }
#endif
  VC_SS(2);
  if (bad && lane == 0) *v.bad_flag = 1;
  // column j of L / L_jj, contiguous over the rows (entries above the diagonal / beyond row D are never read; lanes past the
  // padded row length all write the last padding slot)
  {
    const int slot = lane < ldt - 1 ? lane : ldt - 1;
#pragma unroll
    for (int j = 0; j < DMAX; ++j) Lt[j * ldt + slot] = row[j];
  }
  // delta_s = -L^-T y.  Lt row i is column i of L over L_ii: c_ij = L[j][i] / L[i][i] for j > i, and y_i / L[i][i] at index D:
  // x_i = -y_i / L_ii - sum_{j > i} c_ij x_j.  Lane i keeps its running sum s; the unknowns are resolved four at a time: the four
  // lanes' sums are broadcast (v_readlane, independent of each other), every lane solves the 4 x 4 triangle itself (its six
  // coefficients are wave-uniform LDS reads, requested ahead) and applies the four unknowns to its sum -- one scalar round trip
  // per four unknowns on the dependent chain instead of one per unknown.  A lane inside the block ends up with its own unknown:
  // the terms the broadcast value was still missing are exactly the ones the update adds (c_ij = 0 for j <= i).
  wave_lds_sync();
  VC_SS(3);
  double c[DMAX];
#pragma unroll
  for (int j = 0; j < DMAX; ++j) c[j] = (j < D && lane < D && j > lane) ? Lt[lane * ldt + j] : 0.0;
  double s = (lane < D) ? -Lt[lane * ldt + D] : 0.0;
#pragma unroll
  for (int hi = DMAX; hi > 0; hi -= 4) {
    const int lo = hi >= 4 ? hi - 4 : 0, n = hi - lo;
    double t[4], xb[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) if (q < n) t[q] = readlane_f64(s, lo + q);
#pragma unroll
    for (int q = 3; q >= 0; --q)
      if (q < n) {
        double a = t[q];
#pragma unroll
        for (int r = 3; r > q; --r) if (r < n) a -= ((lo + r < D) ? Lt[(lo + q) * ldt + lo + r] : 0.0) * xb[r];      // oldest unknown first
        xb[q] = a;
      }
#pragma unroll
    for (int q = 0; q < 4; ++q) if (q < n) s -= c[lo + q] * xb[q];
  }
  if (lane < D) x[lane] = s;
  VC_SS(4);
}

// Workgroup-wide factorisation for D > 32.  Only the lower triangle (plus the right-hand-side row D) is kept, packed:
// row i starts at i (i + 1) / 2 -- 129 KB of LDS at D = 178 (8 cameras + IMU + 7 separators) instead of 256 KB.
__device__ __forceinline__ int tri(int i) { return (i * (i + 1)) >> 1; }
// Factorisation: register-tiled, one barrier per two columns (factor_large_tiled below); back-substitution: panels of 16 columns from the
// bottom -- partial sums over the rows below on the 16 x 16 thread grid, the 16 x 16 diagonal block by one wavefront (v_readlane).
// Same packed storage; extra LDS after x: two column images (2 x 192 doubles each, 16-byte aligned), dinv (D).
// (Rounds 3-6 factored in panels of 16 too: diagonal block on one wavefront -- ~400 cycles per pivot --, rows below one per thread, trailing
//  update on the matrix pipe, three barriers per panel; the register-tiled form is 18-20 % faster end to end at D = 67 and D = 115
//  (profiles/r06_ab_reduced_tiled.txt) and a third of the code.  Also measured there and not kept: the diagonal blocks inverted up front so that a
//  panel of the back-substitution is a product -- the inversion costs what the sixteen-step chains did.)
#ifdef VC_REDUCED_STAMPS
#define VC_PH(i) do { if (threadIdx.x == 0) { const long long now_ = (long long)__builtin_readcyclecounter(); ph_[i] += now_ - t_; t_ = now_; } } while (0)
#else
#define VC_PH(i) do { } while (0)
#endif
// (round 6, last part) Register-tiled right-looking Cholesky of the (D + 1) x (D + 1) system [S + damping; g_red^T] for D > 32.  The 256 threads
// form a 16 x 16 grid (tr, tc); thread (tr, tc) OWNS the entries (tr + 16 a, tc + 16 b), b <= a, of the lower triangle and keeps them in
// registers from the load (straight from Sbuf: one memory round trip for the whole matrix, no LDS image of the unfactored system) to the
// end -- NT (NT + 1) / 2 doubles, NT = ceil((D + 1) / 16) <= 12.  A step (two columns, see below) costs ONE workgroup barrier: the columns'
// owners put their unscaled entries into an LDS column image (two images, alternating), everybody reads the pivot block and its own rows' and
// columns' entries, forms the reciprocals itself and updates its tile -- independent FMAs, the block column jb a compile-time constant, so
// that finished block rows / columns cost nothing.  The scaled columns go into the packed triangle M (LDS) -- the factor the
// back-substitution below reads, in the layout the panel form left it in.  The panel form's critical path was one wavefront's
// 16 x 16 factor per panel (~400 cycles per pivot: that wavefront issues every instruction of the step), a row solve and a trailing update
// behind barriers of their own: 75 k of k_reduced's 110 k cycles at D = 67, 170 k of 218 k at D = 115; this form: 51 k / 99 k -- a pair of
// columns is still ~1300 cycles: LDS write -> barrier -> LDS read -> reciprocals -> FMA is a chain of ~130-cycle hops and ~40-cycle
// dependent fp64 operations that four lone wavefronts cannot hide.
template <int NT> __device__ __forceinline__ constexpr int tix(int a, int b) { return a * (a + 1) / 2 + b; }
#ifdef VC_REDUCED_STAMPS
// (profiling builds: the phases of the step of columns 20 / 21, thread 0 -- every stamp behind a full wait, so that it reads when the phase's results exist)
#define VC_MS(i) do { if (j == 20 && tid == 0) { __builtin_amdgcn_s_waitcnt(0); __builtin_amdgcn_sched_barrier(0); s_rst[20 + (i)] = (long long)__builtin_readcyclecounter(); __builtin_amdgcn_sched_barrier(0); } } while (0)
#define VC_MSV(i, val) do { if (j == 20 && tid == 0) { const int sink_ = __builtin_amdgcn_readfirstlane(__double2hiint(val)); asm volatile("" :: "s"(sink_)); s_rst[20 + (i)] = (long long)__builtin_readcyclecounter(); __builtin_amdgcn_sched_barrier(0); } } while (0)
#else
#define VC_MS(i) do { } while (0)
#define VC_MSV(i, val) do { } while (0)
#endif
template <int NT>
__device__ __forceinline__ void factor_large_tiled(const DevView& v, const Ctrl* ct, double* M, double* x, double* cb0, double* cb1, double* dinv) {
  const int tid = threadIdx.x, tr = tid >> 4, tc = tid & 15, D = v.D;
  const double* S = v.Sbuf;
  const double* hd = S + D * D + D;
  double T[NT * (NT + 1) / 2];
  // rows 0 .. D - 1: S's lower triangle; row D: g_red (which follows S in Sbuf: entry (D, k) is S[D D + k]); everything else zero
#pragma unroll
  for (int a = 0; a < NT; ++a)
#pragma unroll
    for (int b = 0; b <= a; ++b) {
      const int i = tr + 16 * a, k = tc + 16 * b;
      const bool in = i <= D && k <= i && k < D;
      const double t = S[in ? i * D + k : 0];
      T[tix<NT>(a, b)] = in ? t : 0.0;
    }
  for (int i = tid; i < D; i += 256) {
    double sc2, dg;
    if (ct->init_scale) { sc2 = jacobi_scale2(hd[i]); v.sscale2[i] = sc2; } else sc2 = v.sscale2[i];
    if (!ct->reuse_diag) { dg = lm_clamped_diag(hd[i], sc2); v.sdiag[i] = dg; } else dg = v.sdiag[i];
    const double lam = dg / (ct->radius * sc2);
    v.slam[i] = lam;
    x[i] = lam;
  }
  __syncthreads();
  if (tr == tc) {
#pragma unroll
    for (int a = 0; a < NT; ++a) { const int i = tr + 16 * a; const double lam = x[i < D ? i : 0]; T[tix<NT>(a, a)] += i < D ? lam : 0.0; }
  }
#ifdef VC_REDUCED_STAMPS
  if (tid == 0) { const int sink_ = __builtin_amdgcn_readfirstlane(__double2hiint(T[0])); asm volatile("" :: "s"(sink_)); s_rst[14] = (long long)__builtin_readcyclecounter(); }
#endif
  // Column steps, TWO columns per barrier.  No masks: an entry whose row or column is <= j + 1 is never read again -- whatever the step does
  // to it stays in entries nobody uses (the upper halves of the diagonal tiles included).  The owners of columns j and j + 1 put their UNSCALED
  // entries a_i, b_i (b not yet updated by column j) side by side into the column image; everybody reads the 2 x 2 pivot block [p; m, b_q] and
  // its own rows' and columns' pairs (one 16-byte LDS read each) and does the small factorisation itself: r1 = 1 / p, b'_i = b_i - a_i (m r1),
  // q = b_q - m (m r1), r2 = 1 / q, then T(i, k) -= a_i (a_k r1) + b'_i (b'_k r2) -- the FMAs of two single steps behind ONE write -> barrier ->
  // read chain (a single step is ~830 cycles at D = 67 of which the tile's FMAs are a tenth).  1 / sqrt(p), 1 / sqrt(q), which only the stored
  // factor needs, run beside the reciprocal chains; the factor's two columns go out coalesced, one row per thread (threads 0 .. 16 NT - 1),
  // straight from the column image.  An odd last column is one single step of the same form.
  // (first cut: one column per barrier, both operands scaled by 1 / sqrt(c_j) behind selects, the owners storing the factor's column through
  //  tri(i): 62 k cycles for the factorisation at D = 67 (75 k in the panel form); without the selects and with coalesced stores: 56 k)
  bool bad = false;
  const int wi = tid < 16 * NT ? tid : 16 * NT - 1, triw = tri(wi);
  typedef double __attribute__((ext_vector_type(2))) v2d_;
#pragma unroll
  for (int jb = 0; jb < NT; ++jb) {
    const int jn = min(16, D - 16 * jb);            // (columns of this block column; <= 0 behind the matrix)
    const int npair = jn > 0 ? jn >> 1 : 0;
#pragma nounroll
    for (int pc = 0; pc < npair; ++pc) {
      const int j = 16 * jb + 2 * pc;
      double* cb = (pc & 1) ? cb1 : cb0;             // (eight pairs per full block column: the parity carries over)
      VC_MS(0);
      if ((tc >> 1) == pc) {
        const int sl = tc & 1;
#pragma unroll
        for (int a = jb; a < NT; ++a) cb[2 * (tr + 16 * a) + sl] = T[tix<NT>(a, jb)];
      }
      VC_MS(1);
      __syncthreads();
      VC_MS(2);
      const v2d_* cb2 = reinterpret_cast<const v2d_*>(cb);
      const v2d_ pv0 = cb2[j], pv1 = cb2[j + 1], cw = cb2[wi];
      v2d_ ri[NT], ck[NT];
#pragma unroll
      for (int b = jb; b < NT; ++b) ck[b] = cb2[tc + 16 * b];
#pragma unroll
      for (int a = jb; a < NT; ++a) ri[a] = cb2[tr + 16 * a];
      const double p = pv0.x, m = pv1.x, bq = pv1.y;
      const bool ok1 = p > 0.0;
      const double ps = ok1 ? p : 1.0;              // (a pivot that is not positive: identity column, the pass is flagged -- as the panel form)
      VC_MSV(3, ri[NT - 1].x);
      const double r1 = fast_rcp(ps), ip1 = fast_rsqrt(ps);
      const double mr = m * r1;
      const double q = bq - m * mr;
      const bool ok2 = q > 0.0;
      const double qs = ok2 ? q : 1.0;
      const double r2 = fast_rcp(qs), ip2 = fast_rsqrt(qs);
      bad |= !ok1 || !ok2;
      VC_MSV(4, r2);
#pragma unroll
      for (int b = jb; b < NT; ++b) { const double bk = ck[b].y - ck[b].x * mr; ck[b].x *= r1; ck[b].y = bk * r2; }
#pragma unroll
      for (int a = jb; a < NT; ++a) ri[a].y -= ri[a].x * mr;
#pragma unroll
      for (int a = jb; a < NT; ++a)
#pragma unroll
        for (int b = jb; b <= a; ++b) T[tix<NT>(a, b)] -= ri[a].x * ck[b].x + ri[a].y * ck[b].y;
      VC_MSV(5, T[tix<NT>(NT - 1, NT - 1)]);
      // the factor's columns j, j + 1 below the diagonal (row D: the forward-substituted right-hand side) and the two diagonal entries
      if (tid > j && tid <= D) M[triw + j] = cw.x * ip1;
      if (tid > j + 1 && tid <= D) M[triw + j + 1] = (cw.y - cw.x * mr) * ip2;
      if (tid == j) { M[triw + j] = ok1 ? p * ip1 : 1.0; dinv[j] = ip1; }
      if (tid == j + 1) { M[triw + j + 1] = ok2 ? q * ip2 : 1.0; dinv[j + 1] = ip2; }
      VC_MS(6);
    }
    if (jn > 0 && (jn & 1)) {                        // the matrix's last column (D odd): a single step
      const int jc = jn - 1, j = 16 * jb + jc;
      double* cb = (npair & 1) ? cb1 : cb0;
      if (tc == jc) {
#pragma unroll
        for (int a = jb; a < NT; ++a) cb[tr + 16 * a] = T[tix<NT>(a, jb)];
      }
      __syncthreads();
      const double cj = cb[j], cw = cb[wi];
      double ci[NT], ck[NT];
#pragma unroll
      for (int b = jb; b < NT; ++b) ck[b] = cb[tc + 16 * b];
#pragma unroll
      for (int a = jb; a < NT; ++a) ci[a] = cb[tr + 16 * a];
      const bool ok = cj > 0.0;
      bad |= !ok;
      const double cjs = ok ? cj : 1.0;
      const double r = fast_rcp(cjs), ipiv = fast_rsqrt(cjs);
#pragma unroll
      for (int b = jb; b < NT; ++b) ck[b] *= r;
#pragma unroll
      for (int a = jb; a < NT; ++a)
#pragma unroll
        for (int b = jb; b <= a; ++b) T[tix<NT>(a, b)] -= ci[a] * ck[b];
      if (tid > j && tid <= D) M[triw + j] = cw * ipiv;
      if (tid == j) { M[triw + j] = ok ? cj * ipiv : 1.0; dinv[j] = ipiv; }
    }
  }
  if (bad && tid == 0) v.flags[5 + 2 * v.par] = 1;
  __syncthreads();
}
__device__ __forceinline__ void solve_large_tiled(const DevView& v, const Ctrl* ct, double* M, double* x) {
  const int tid = threadIdx.x, lane = tid & 63, D = v.D;
#ifdef VC_REDUCED_STAMPS
  long long ph_[6] = {0, 0, 0, 0, 0, 0}, t_ = (long long)__builtin_readcyclecounter();      // - | load + factorisation | - | - | back-subst sums | back-subst solve
#endif
  double* Lp = x + (D + 1);                      // column image 0 of the factorisation: two columns side by side, 2 x 192 doubles, 16-byte aligned
  if (reinterpret_cast<uintptr_t>(Lp) & 8) ++Lp;
  double* red = Lp + 384;                        // column image 1; the back-substitution's 16 x 16 partial sums
  double* dinv = red + 384;
  {
    const int nT = (D + 1 + 15) >> 4;
    switch (nT) {
      case 3: factor_large_tiled<3>(v, ct, M, x, Lp, red, dinv); break;
      case 4: factor_large_tiled<4>(v, ct, M, x, Lp, red, dinv); break;
      case 5: factor_large_tiled<5>(v, ct, M, x, Lp, red, dinv); break;
      case 6: factor_large_tiled<6>(v, ct, M, x, Lp, red, dinv); break;
      case 7: factor_large_tiled<7>(v, ct, M, x, Lp, red, dinv); break;
      case 8: factor_large_tiled<8>(v, ct, M, x, Lp, red, dinv); break;
      case 9: factor_large_tiled<9>(v, ct, M, x, Lp, red, dinv); break;
      case 10: factor_large_tiled<10>(v, ct, M, x, Lp, red, dinv); break;
      case 11: factor_large_tiled<11>(v, ct, M, x, Lp, red, dinv); break;
      default: factor_large_tiled<12>(v, ct, M, x, Lp, red, dinv); break;
    }
    VC_PH(1);
  }
  // ---- delta_s = -L^-T y (y = row D), panels from the bottom ----------------------------------------------------------
  for (int i = tid; i < D; i += 256) x[i] = -M[tri(D) + i];
  __syncthreads();
  const int last = ((D - 1) / 16) * 16;
  for (int p0 = last; p0 >= 0; p0 -= 16) {
    const int nb = min(16, D - p0), r0 = p0 + nb;
    {   // t_j = x_j - sum_{i >= r0} L[i][p0 + j] x_i : 16 columns x 16 partial sums
      const int jcol = tid & 15, part = tid >> 4;
      double acc = 0.0;
      if (jcol < nb) for (int i = r0 + part; i < D; i += 16) acc += M[tri(i) + p0 + jcol] * x[i];
      red[part * 16 + jcol] = acc;
    }
    __syncthreads();
    VC_PH(4);
    if (tid < 64) {
      double t = 0.0;
      if (lane < nb) {
        t = x[p0 + lane];
#pragma unroll
        for (int q = 0; q < 16; ++q) t -= red[q * 16 + lane];
      }
      const double di = (lane < nb) ? dinv[p0 + lane] : 1.0;
      // the lane's column of the diagonal block, requested before the dependent chain (round 6: as a read inside every step the chain was an
      // LDS round trip per unknown -- 3.7k cycles per panel; now a multiply, two v_readlane and an FMA)
      // (the unknowns four at a time, as solve_small_wave -- every lane solving the 4 x 4 triangle itself from wave-uniform LDS reads -- was
      //  measured here and is slower: 56 LDS reads per panel instead of 33, panels 3.4 k -> 5.3 k cycles)
      double Lc[16];
#pragma unroll
      for (int j = 0; j < 16; ++j) { const bool in = j < nb && lane < j; const double t = M[in ? tri(p0 + j) + p0 + lane : 0]; Lc[j] = in ? t : 0.0; }
      __builtin_amdgcn_sched_barrier(0);      // (the reads are issued here, not sunk to their uses)
      double z = 0.0;
#pragma unroll
      for (int j = 15; j >= 0; --j) {
        if (j < nb) {                                  // wave-uniform
          const double zj = readlane_f64(t * di, j);
          if (lane == j) z = zj;
          t -= Lc[j] * zj;
        }
      }
      if (lane < nb) x[p0 + lane] = z;
    }
    __syncthreads();
    VC_PH(5);
  }
#ifdef VC_REDUCED_STAMPS
  if (threadIdx.x == 0) for (int i = 0; i < 6; ++i) s_rst[8 + i] = ph_[i];
#endif
}

__device__ __forceinline__ void reduced_solve_phase(const DevView& v, const Ctrl* ct, double* dyn, double* red /* 6 x 256 */, const double* s_cam,
                                    double pre_sc2, double pre_dg, const double* x2_noobs, const CamDesc* cd /* LDS copy of v.cd */,
                                    const double* Sb /* v.Sbuf or its LDS image */, double pre_imu, const int* ipc /* LDS copy of v.imu_param_col */) {
  const int tid = threadIdx.x, D = v.D, cur = ct->cur;
  double* x;
  VC_STAMP(4);
  if (D <= kSmallD) {
    x = dyn + (kSmallD + 1) * (kSmallD + 2);
    if (tid < 64 && D > 0) {
      // (every column up to DMAX is eliminated whether the matrix has it or not: instances close to the common widths)
      const SmallSolveArgs a = {D, v.sscale2, v.sdiag, v.slam, v.flags + 5 + 2 * v.par, v.dbg};
      if (D <= 16) solve_small_wave<16>(a, ct, tid, dyn, x, pre_sc2, pre_dg, Sb, red);
      else if (D <= 24) solve_small_wave<24>(a, ct, tid, dyn, x, pre_sc2, pre_dg, Sb, red);
      else if (D <= 28) solve_small_wave<28>(a, ct, tid, dyn, x, pre_sc2, pre_dg, Sb, red);
      else if (D <= 30) solve_small_wave<30>(a, ct, tid, dyn, x, pre_sc2, pre_dg, Sb, red);
      else solve_small_wave<32>(a, ct, tid, dyn, x, pre_sc2, pre_dg, Sb, red);
    }
    __syncthreads();
  } else {
    x = dyn + tri(D + 1) + (D + 1);
    solve_large_tiled(v, ct, dyn, x);
  }
  VC_STAMP(5);
  const bool small = D <= kSmallD;      // the one-wavefront solve left damping and g_s in LDS behind x
  const double* gs = small ? x + 2 * (kSmallD + 1) : v.Sbuf + (size_t)D * D + 2 * D;
  const double* lamv = small ? x + (kSmallD + 1) : v.slam;
  if (v.tail_deferred) {
    // (round 6) the back-substitution's launch carries the rest (reduced_tail, one extra workgroup): this kernel -- one workgroup the whole
    // chip waits for -- ends with the step and the trial IMU parameters (which the second stream's k_imu_block(trial) starts from)
    for (int i = tid; i < D; i += 256) v.delta_s[i] = x[i];
    if (v.imu_on && (tid >> 6) == (D <= 64 ? 0 : 1) && (tid & 63) < 16) {
      const int a = tid & 63, col = a < 15 ? ipc[a] : -1;
      v.imus[1 - cur][a] = pre_imu + (col >= 0 ? x[col] : 0.0);      // (g(2) b(6) sf(6) toff(1): plain additive parameters; entry 15: padding)
    }
    return;
  }
  reduced_tail(v, cur, x, gs, lamv, s_cam, cd, ipc, pre_imu, x2_noobs, red, true, true);
}

// mode 0: phase A + phase B in one launch (single process); 1: phase A only (an all-reduce of Sbuf follows);
// 2: phase B only
__global__ __launch_bounds__(256) void k_reduced(DevView v, int mode) {
  extern __shared__ __attribute__((aligned(16))) double dyn[];   // phase A: FinalLds; phase B: the matrix (the phases do not overlap)
  __shared__ double red[6 * 256];
  __shared__ double s_cam[kMaxCams * kCamStride];     // accepted camera records: requested at kernel entry, used by the tail
  __shared__ double s_x2;
  __shared__ CamDesc s_cd[kMaxCams];     // the kernel-argument table costs a scalar memory round trip per (dynamically indexed) access
  __shared__ int s_ipc[16];              // ... and so does DevView::imu_param_col (as 15 s_load_dword, one per use, it was 3.6k cycles of the tail)
  const Ctrl* ct = v.ctrl;
  __shared__ double s_S[kSmallD * kSmallD + 3 * kSmallD + 2];      // single process, D <= kSmallD: the reduced system stays in LDS between the phases
  // early Gram: [Y | z] rows of the chain's top-level frames, behind phase A's record in the dynamic region (static LDS is at its limit
  // where the packed matrix of a D = 178 system takes 137 KB of the dynamic one)
  double* s_top = dyn + (sizeof(FinalLds) + 7) / 8;
  const bool early = v.gram_top_stride > 0 && mode == 0 && v.D <= kEarlyTopD;
  const int top_rows = early ? 9 * min(7, (v.n_frames - 1) / v.gram_top_stride + 1) : 0;
  // the top-level frames' rows (final since the launch before the partial sums): requested first -- together with the control record,
  // not behind it --, their latency under everything below
  double tin[9];
  const double* top_src = early ? v.cW : v.Sbuf;      // (no chain: every lane reads the always-present first entry of Sbuf and drops it)
#pragma unroll
  for (int u = 0; u < 9; ++u) {
    const int idx = threadIdx.x + 256 * u, r = idx / kTopLd, c = idx - r * kTopLd;
    const bool in = early && idx < 64 * kTopLd && r < top_rows && c <= v.D;
    const double x = top_src[in ? ((size_t)(r / 9) * v.gram_top_stride * 9 + (r % 9)) * v.ldx + c : 0];
    tin[u] = in ? x : 0.0;
  }
  if (ct->done) { if (threadIdx.x == 0 && mode != 1) signal_flag(v, 1); return; }
  if (threadIdx.x < kMaxCams) s_cd[threadIdx.x] = v.cd[threadIdx.x];
  if (threadIdx.x >= 64 && threadIdx.x < 64 + 15) s_ipc[threadIdx.x - 64] = v.imu_param_col[threadIdx.x - 64];
  if (early) {
#pragma unroll
    for (int u = 0; u < 9; ++u) { const int idx = threadIdx.x + 256 * u; if (idx < 64 * kTopLd) s_top[idx] = tin[u]; }
  }
  double pre_sc2 = 1.0, pre_dg = 1.0;      // damping inputs of the small solve: requested now, consumed after phase A
  double pre_imu = 0.0;                    // accepted IMU parameters (lane a of the wavefront whose thread forms the trial ones): the tail's
  if (mode != 1) {
    for (int i = threadIdx.x; i < v.n_cams * kCamStride; i += 256) s_cam[i] = v.cams[ct->cur][i];
    if (v.D <= kSmallD && (int)threadIdx.x < v.D) { pre_sc2 = v.sscale2[threadIdx.x]; pre_dg = v.sdiag[threadIdx.x]; }
    if (v.imu_on && (int)(threadIdx.x >> 6) == (v.D <= 64 ? 0 : 1) && (threadIdx.x & 63) < 16) pre_imu = v.imus[ct->cur][threadIdx.x & 63];
  }
  const bool s_in_lds = mode == 0 && v.D <= kSmallD;
  if (s_in_lds) {
    schur_final_phase(v, ct->cur, *reinterpret_cast<FinalLds*>(dyn), &s_x2, s_cd, s_ipc, s_S, true, early ? s_top : nullptr, top_rows);
    __syncthreads();
    // Sbuf keeps its meaning for k_final (cost slot) and the parity hooks: written back off the critical path
    for (int e = threadIdx.x; e < v.D * v.D + 3 * v.D + 2; e += 256) v.Sbuf[e] = s_S[e];
  } else if (mode != 2) { schur_final_phase(v, ct->cur, *reinterpret_cast<FinalLds*>(dyn), &s_x2, s_cd, s_ipc, v.Sbuf, false); __syncthreads(); }
  if (mode != 1) reduced_solve_phase(v, ct, dyn, red, s_cam, pre_sc2, pre_dg, mode == 0 ? &s_x2 : nullptr, s_cd, s_in_lds ? s_S : v.Sbuf, pre_imu, s_ipc);
  if (mode != 1) { __syncthreads(); if (threadIdx.x == 0) signal_flag(v, 1); }      // the trial IMU parameters exist (stream B's deltas wait for this)
#ifdef VC_REDUCED_STAMPS
  VC_STAMP(7);
  __syncthreads();
  if (threadIdx.x < 32) v.dbg[threadIdx.x] = s_rst[threadIdx.x];
#endif
}

}  // namespace vc
