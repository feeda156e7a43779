// vci_chain_fwd.hpp -- k_chain_fwd: one level of the partitioned chain elimination: a wavefront eliminates the interior frames of a group of 8
// (L, X_s = L^-1 C, X_n = L^-1 B, Y = L^-1 [W | g]); the group's first frame survives to the next level.
// Kernel fragment of vc_imu_kernels.hip alone (defines __global__ symbols; included there in stage order; not for host harnesses).
#pragma once
#include <hip/hip_runtime.h>
#include "vc_math.hpp"
#include "vc_device.h"
#include "vc_kutil.hpp"

namespace vc {

// ------------------------------------------------------------------------------------------ chain elimination
// The frame unknowns (pose 6 + velocity 3) form a block-tridiagonal chain with a dense border (the shared parameters and
// the right-hand side).  Every frame owns one IMAGE of 9 rows (cW, row stride ldx): columns 0..D the border [W | g], then
// from column ldw the three 9 x 9 blocks [C | A | B] -- C the coupling to the left separator (fill-in; zero to start
// with), A the frame's own block, B the coupling to the next active frame (rows = this frame).
// The chain is factored by nested partitioning: at level l the active frames are those with index 0 (mod s), s = m^l;
// they are cut into groups of m -- the first frame of a group is its LEFT SEPARATOR and stays active, the other m - 1 (the
// interior) are eliminated by ONE wavefront, sequentially, left to right, with lane = image column throughout:
//   * factor A = L L^T (nine lanes, lane = row, pivots through v_readlane; the factor goes to LDS);
//   * every lane solves L x = (its column); the solved C and B columns [X_s | X_n] (18 columns) go to LDS, the solved
//     image replaces the frame's image in HBM (the A columns receive L itself): that is all the back-substitution needs;
//   * every lane forms out = [X_s | X_n]^T x: rows 9..17 update the lane's column of the NEXT frame's image (which the
//     lane keeps in registers for the next elimination; A's columns go to LDS for the next factorisation), rows 0..8
//     accumulate the group's update of the left separator.
// The last interior's "next" is the right separator, which belongs to the neighbouring group: its update goes to a side
// image (rX, double-buffered by level parity) and is folded in when that frame is loaded or written at the next level.
// A few levels (N = 2000, m = 8: 2000 -> 250 -> 32 -> 4) and a top level that eliminates what is left replace the
// 2 log2(N) launches of cyclic reduction by log_m(N) + 1, with (m - 1) log_m(N) dependent eliminations.
constexpr int kXsLd = 20;           // row stride of the [X_s | X_n] LDS image
// phase stamps of the first group of level 0 (profiling builds only, -DVC_CHAIN_STAMPS): 100 MHz s_memrealtime ticks in dbg[0..31]
#ifdef VC_CHAIN_STAMPS
#define CSTAMP(i) do { if (group == 0 && lvl == 0 && threadIdx.x == 0 && (i) < 32) v.dbg[i] = (long long)__builtin_amdgcn_s_memrealtime(); } while (0)
#else
#define CSTAMP(i) do { } while (0)
#endif
// NW > 1: the group's columns are spread over NW wavefronts of one workgroup instead of several columns per lane (column
// c = lane + 64 (wave + NW ci)).  Every wavefront factors A itself (its own copy of L in LDS: nine lanes, a microsecond), the
// solved [X_s | X_n] columns and the next frame's A are exchanged through the shared LDS images behind workgroup barriers.  For
// wide borders (D > 36) this replaces columns per lane, which cost 25 us per elimination at three columns (256 VGPR + AGPR
// copies) against a few us here; the columns-per-lane instances stay for A/B runs (chain_levels, vc_imu_kernels.hip).
// One group of one level: `group` its index, `wave` the wavefront's index inside the group (0 .. NW - 1), the LDS images
// XS (9 x kXsLd), An (81), Ls_all (NW x 81) the group's own.  NW > 1: all wavefronts of the workgroup belong to the group.
template <int CPL, int NW>          // columns per lane x wavefronts: D + 1 + 27 <= 64 CPL NW
__device__ __forceinline__ void chain_fwd_group(const DevView& v, int s, int m, int top, int lvl, int group, int wave, double* XS, double* An, double* Ls_all) {
  auto group_sync = [&]() { if (NW > 1) __syncthreads(); else wave_lds_sync(); };
  CSTAMP(0);
  // the control record is requested here and looked at after the first frame's image has been requested as well: a finished
  // solve costs a few wasted loads, a running one saves the record's round trip at the head of every level
  const int done = v.ctrl->done;
  if (lvl == 1 && blockIdx.x == 0 && threadIdx.x == 0) signal_started(v, 7);      // the bottom level is complete: this launch runs (the weight update waits for it)
  const int lane = threadIdx.x & 63;
  const int N = v.n_frames, D = v.D, ldw = v.ldw, ldx = v.ldx, nW = D + 1, ncol = nW + 27;
  const long gs = (long)m * s;
  const int a = top ? -1 : (int)(group * gs);
  const int first = top ? 0 : a + s;
  const bool pend = lvl > 0;                                   // right contributions of level lvl - 1 are waiting
  const double* rp = v.rX[(lvl + 1) & 1];
  double* rw = v.rX[lvl & 1];
  const size_t isz = (size_t)9 * ldx;
  // role of each of the lane's columns: 0 border (W | g), 1 C, 2 A, 3 B, 4 none
  int role[CPL], pc[CPL], sub[CPL];
#pragma unroll
  for (int ci = 0; ci < CPL; ++ci) {
    const int c = lane + 64 * (wave + NW * ci), e = c - nW;
    role[ci] = c < nW ? 0 : (e < 9 ? 1 : e < 18 ? 2 : e < 27 ? 3 : 4);
    pc[ci] = c < nW ? c : (c < ncol ? ldw + e : 0);
    sub[ci] = e < 9 ? e : e < 18 ? e - 9 : e - 18;            // column inside the 9 x 9 block
  }
  if (first >= N) {            // a separator without interior frames: only its pending right contribution is folded in
    if (!done && !top && a < N) {
#pragma unroll
      for (int ci = 0; ci < CPL; ++ci) {
        double* img = v.cW + (size_t)a * isz + pc[ci];
        if ((role[ci] == 0 || role[ci] == 2) && pend && a > 0) {
#pragma unroll
          for (int k = 0; k < 9; ++k) img[k * ldx] += rp[(size_t)(a / s) * isz + k * ldx + pc[ci]];
        } else if (role[ci] == 3) {
#pragma unroll
          for (int k = 0; k < 9; ++k) img[k * ldx] = 0.0;
        }
      }
    }
    return;
  }
  const int q = top ? (N - 1) / s + 1 : min(m - 1, (N - 1 - first) / s + 1);      // frames this wavefront eliminates
  double xin[CPL][9], dacc[CPL][9];
#pragma unroll
  for (int ci = 0; ci < CPL; ++ci)
#pragma unroll
    for (int k = 0; k < 9; ++k) dacc[ci][k] = 0.0;
  // ---- the first frame: its image columns to the lanes (C = B_a^T, a row of the separator's B block), A to LDS; the
  // second frame's columns are requested in the same breath (o / op: the next frame's image and its pending update)
  // four columns per lane (D > 164) do not leave registers for the pending values as well: they are read where they are used
  constexpr bool kLateOp = CPL >= 4;
  double o[CPL][9], op[kLateOp ? 1 : CPL][9];
  auto request_next = [&](int e, int i) {
    const int n = e + s;
    const bool load_n = (n < N) && !(!top && (i == m - 2));        // wave-uniform
    if (!load_n) return;                                            // (o / op are not read then)
    const double* img = v.cW + (size_t)n * isz;
    // unconditional loads: idle lanes (role 4) read column 0, their values are never used
#pragma unroll
    for (int ci = 0; ci < CPL; ++ci)
#pragma unroll
      for (int k = 0; k < 9; ++k) o[ci][k] = img[k * ldx + pc[ci]];
    if (pend && !kLateOp) {
      const double* rpn = rp + (size_t)(n / s) * isz;
#pragma unroll
      for (int ci = 0; ci < CPL; ++ci)
#pragma unroll
        for (int k = 0; k < 9; ++k) op[ci][k] = rpn[k * ldx + pc[ci]];
    }
  };
#pragma unroll
  for (int ci = 0; ci < CPL; ++ci)
#pragma unroll
    for (int k = 0; k < 9; ++k) { o[ci][k] = 0.0; if (!kLateOp) op[ci][k] = 0.0; }
  {
    const bool pe = pend && first > 0;
    const double* img = v.cW + (size_t)first * isz;
    const double* rpe = rp + (size_t)(first / s) * isz;
    double x0[CPL][9], xp[CPL][9];
#pragma unroll
    for (int ci = 0; ci < CPL; ++ci) {
      if (role[ci] == 1) {
#pragma unroll
        for (int k = 0; k < 9; ++k) { x0[ci][k] = (a >= 0) ? v.cW[(size_t)a * isz + sub[ci] * ldx + ldw + 18 + k] : 0.0; xp[ci][k] = 0.0; }
      } else {
#pragma unroll
        for (int k = 0; k < 9; ++k) { x0[ci][k] = (role[ci] < 4) ? img[k * ldx + pc[ci]] : 0.0; xp[ci][k] = (pe && role[ci] < 4) ? rpe[k * ldx + pc[ci]] : 0.0; }
      }
    }
    request_next(first, 0);
    if (done) return;
    CSTAMP(1);
#pragma unroll
    for (int ci = 0; ci < CPL; ++ci) {
#pragma unroll
      for (int k = 0; k < 9; ++k) xin[ci][k] = x0[ci][k] + xp[ci][k];
      if (role[ci] == 2) {
#pragma unroll
        for (int k = 0; k < 9; ++k) An[k * 9 + sub[ci]] = xin[ci][k];
      }
    }
  }
  for (int i = 0; i < q; ++i) {
    const int e = first + i * s, n = e + s;
    const bool has_n = n < N;
    const bool n_sep = !top && (i == m - 2);                   // the next frame is the right separator (another group's)
    if (i > 0) request_next(e, i);       // the next frame's columns: requested now, used after the factorisation and the solve
    group_sync();                        // the frame's A block (LDS) is complete
    CSTAMP(2 + 4 * i);
    // ---- A = L L^T in every lane, from registers (see k_chain_fwd2: before, nine lanes factored through v_readlane and the factor
    // went through LDS); the triangular solves take L from registers
    double Lr[45], dinv[9];
    {
#pragma unroll
      for (int ii = 0; ii < 9; ++ii)
#pragma unroll
        for (int j = 0; j <= ii; ++j) Lr[ii * (ii + 1) / 2 + j] = An[ii * 9 + j];
      bool bad = false;
#pragma unroll
      for (int j = 0; j < 9; ++j) {
        double d = Lr[j * (j + 1) / 2 + j];
        const bool ok = d > 0.0;
        bad |= !ok;
        d = ok ? d : 1.0;
        const double ip = fast_rsqrt(d);
        dinv[j] = ip;
        Lr[j * (j + 1) / 2 + j] = d * ip;
#pragma unroll
        for (int ii = j + 1; ii < 9; ++ii) Lr[ii * (ii + 1) / 2 + j] *= ip;
#pragma unroll
        for (int ii = j + 1; ii < 9; ++ii)
#pragma unroll
          for (int k = j + 1; k <= ii; ++k) Lr[ii * (ii + 1) / 2 + k] -= Lr[ii * (ii + 1) / 2 + j] * Lr[k * (k + 1) / 2 + j];
      }
      if (bad) {               // uniform (every lane holds the same numbers): the frame gets an identity block, the pass is flagged
        if (lane == 0 && wave == 0) atomicAdd(&v.flags[4 + 2 * v.par], 1);
#pragma unroll
        for (int ii = 0; ii < 9; ++ii) {
          dinv[ii] = 1.0;
#pragma unroll
          for (int j = 0; j <= ii; ++j) Lr[ii * (ii + 1) / 2 + j] = (ii == j) ? 1.0 : 0.0;
        }
      }
    }
    CSTAMP(3 + 4 * i);
    // ---- forward solves, lane = column; the image of e becomes [Y | z | X_s | L | X_n]
    double x[CPL][9];
#pragma unroll
    for (int ci = 0; ci < CPL; ++ci) {
      // column-oriented: x_k is final after k updates, the updates of one column are independent of each other
#pragma unroll
      for (int r = 0; r < 9; ++r) x[ci][r] = xin[ci][r];
#pragma unroll
      for (int k = 0; k < 9; ++k) {
        x[ci][k] *= dinv[k];
#pragma unroll
        for (int r = k + 1; r < 9; ++r) x[ci][r] -= Lr[r * (r + 1) / 2 + k] * x[ci][k];
      }
      // an A lane has solved L x = A e_sub: x = row `sub` of L; the image wants column `sub` -- the nine lanes (of whichever
      // wavefronts) transpose through the group's LDS image behind the barrier of the [X_s | X_n] exchange
      if (role[ci] == 2) {
#pragma unroll
        for (int k = 0; k < 9; ++k) Ls_all[k * 9 + sub[ci]] = (k <= sub[ci]) ? x[ci][k] : 0.0;
      }
      if (role[ci] == 0 || role[ci] == 1 || role[ci] == 3) {
        double* img = v.cW + (size_t)e * isz + pc[ci];
#pragma unroll
        for (int k = 0; k < 9; ++k) img[k * ldx] = x[ci][k];
      }
      if (role[ci] == 1 || role[ci] == 3) {
        const int xc = sub[ci] + (role[ci] == 3 ? 9 : 0);
#pragma unroll
        for (int k = 0; k < 9; ++k) XS[k * kXsLd + xc] = x[ci][k];
      }
    }
    group_sync();                        // [X_s | X_n] is complete
    CSTAMP(4 + 4 * i);
    // ---- Schur updates: out[r] = sum_k [X_s | X_n][k][r] * (column)[k]; the A columns are driven by X_n's columns
#pragma unroll
    for (int ci = 0; ci < CPL; ++ci) {
      if (role[ci] == 2) {
        double* img = v.cW + (size_t)e * isz + pc[ci];
#pragma unroll
        for (int k = 0; k < 9; ++k) img[k * ldx] = Ls_all[sub[ci] * 9 + k];      // L[k][sub] (zero above the diagonal)
#pragma unroll
        for (int k = 0; k < 9; ++k) x[ci][k] = XS[k * kXsLd + 9 + sub[ci]];
      }
      double out[18];
#pragma unroll
      for (int r = 0; r < 18; ++r) out[r] = 0.0;
#pragma unroll
      for (int k = 0; k < 9; ++k) {
        const double xk = x[ci][k];
#pragma unroll
        for (int r = 0; r < 18; ++r) out[r] += XS[k * kXsLd + r] * xk;
      }
#pragma unroll
      for (int r = 0; r < 9; ++r) dacc[ci][r] += out[r];
      if (has_n) {
        if (n_sep) {
          if (role[ci] < 4) {
            double* ri = rw + (size_t)(n / gs) * isz + pc[ci];
            const bool keep = role[ci] == 0 || role[ci] == 2;
#pragma unroll
            for (int k = 0; k < 9; ++k) ri[k * ldx] = keep ? -out[9 + k] : 0.0;
          }
          if (role[ci] == 3 && a >= 0) {                      // the separator's coupling to the right separator at the next level
            double* img = v.cW + (size_t)a * isz + pc[ci];
#pragma unroll
            for (int k = 0; k < 9; ++k) img[k * ldx] = -out[k];
          }
        } else {
          if (kLateOp) {
            const double* rpn = rp + (size_t)(n / s) * isz + pc[ci];
#pragma unroll
            for (int k = 0; k < 9; ++k) xin[ci][k] = (o[ci][k] + (pend ? rpn[k * ldx] : 0.0)) - (role[ci] == 3 ? 0.0 : out[9 + k]);
          } else {
#pragma unroll
            for (int k = 0; k < 9; ++k) xin[ci][k] = (o[ci][k] + op[ci][k]) - (role[ci] == 3 ? 0.0 : out[9 + k]);
          }
          if (role[ci] == 2) {
#pragma unroll
            for (int k = 0; k < 9; ++k) An[k * 9 + sub[ci]] = xin[ci][k];
          }
        }
      }
    }
    CSTAMP(5 + 4 * i);
  }
  CSTAMP(30);
  // ---- the left separator absorbs its group (and the right contribution it received one level down)
  if (a >= 0) {
    const bool chain_ends = !(q == m - 1 && first + q * s < N);
    const bool pa = pend && a > 0;
    const double* rpa = rp + (size_t)(a / s) * isz;
#pragma unroll
    for (int ci = 0; ci < CPL; ++ci) {
      if (role[ci] == 0 || role[ci] == 1) {                    // the C lanes carry the update of A's columns
        const int pcd = role[ci] == 1 ? ldw + 9 + sub[ci] : pc[ci];
        double* img = v.cW + (size_t)a * isz + pcd;
#pragma unroll
        for (int k = 0; k < 9; ++k) img[k * ldx] += (pa ? rpa[k * ldx + pcd] : 0.0) - dacc[ci][k];
      } else if (role[ci] == 3 && chain_ends) {
        double* img = v.cW + (size_t)a * isz + pc[ci];
#pragma unroll
        for (int k = 0; k < 9; ++k) img[k * ldx] = 0.0;
      }
    }
  }
}

template <int CPL, int NW>
__global__ __launch_bounds__(64 * NW) void k_chain_fwd(DevView v, int s, int m, int top, int lvl) {
  __shared__ __attribute__((aligned(16))) double XS[9 * kXsLd];
  __shared__ double An[81];
  __shared__ double Ls_all[NW * 81];
  chain_fwd_group<CPL, NW>(v, s, m, top, lvl, (int)blockIdx.x, (int)(threadIdx.x >> 6), XS, An, Ls_all);
}

}  // namespace vc
