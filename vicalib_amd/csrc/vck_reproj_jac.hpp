// vck_reproj_jac.hpp -- k_reproj_jac: the vision sweep.
// One wavefront per (frame,camera) tile: closed-form unique-column Jacobian rows per corner (lane = corner), rows staged in wave-private
// LDS, tile Gram block G = sum w u^T u accumulated on the matrix pipe.
// Kernel fragment: defines __global__ symbols, so it belongs to exactly ONE translation unit -- vc_kernels.hip, which includes the
// fragments in stage order.  Not one of the VC_HD arithmetic headers (vc_math.hpp, ..): host harnesses cannot include it.
#pragma once
#include <hip/hip_runtime.h>
#include "vc_math.hpp"
#include "vc_device.h"
#include "vc_kutil.hpp"

namespace vc {

// ------------------------------------------------------------------------------------------ Jacobian sweep
// One wavefront sweeps one tile.  Per pass of 64 corners: lane = corner computes its two unique-column rows into the
// wave-private LDS image; the Gram block G += u^T u then accumulates on the matrix pipe, four rows (two corners) per step.
//
// The step uses v_mfma_f64_4x4x4_f64 (four independent 4x4x4 blocks per instruction), not the 16x16x4 shape.  Measured on
// MI355X (tools/probe/mfma_f64_probe.hip): the 16x16x4 f64 MFMA has ~300 cycles latency and sustains 49 TF/s, the 4x4x4
// one ~40 cycles and 75 TF/s; f64 MFMA and f64 VALU work do NOT overlap (one shared DP datapath), so what counts is the
// total number of f64 operations -- and the symmetric 16x16 block only needs its upper 4x4 sub-blocks.
// Lane layout of the 4x4x4 instruction (tools/probe/mfma_layout_probe.hip): lane = 16 k + 4 b + i for A_b[i][k],
// 16 k + 4 b + j for B_b[k][j], 16 i + 4 b + j for D_b[i][j].  With k = row of the 4-row group and column
// 4 X_b + (lane & 3) read from that row, block b of an instruction accumulates the sub-block (I_b, J_b) of G:
//   all models : A = pattern (0,1,2,3) for every instruction (one LDS read, also the B operand of the diagonal blocks)
//   <= 12 used columns (fov, linear; 3 block columns): 2 instructions -- diagonal (0,0)(1,1)(2,2)(3,3) and, with
//                A = (0,0,1,3), B = (1,2,2,3): (0,1)(0,2)(1,2)(3,3)           [3 LDS reads per group]
//   otherwise  : 3 instructions -- B = A rotated by 0, 1, 2 blocks: diagonal, (0,1)(1,2)(2,3)(3,0), (0,2)(1,3)(2,0)(3,1)
template <int MODEL>
__device__ __forceinline__ double jac_tile_body(const DevView& v, const double* pose, const double* cam, double mult, int tile, int lane,
                                                double* wl, double* G, int off_in, int cnt_in /* corner range if known (cnt_in >= 0) */) {
  constexpr int nk = MODEL == kFov ? 5 : MODEL == kPoly2 ? 6 : MODEL == kPoly3 ? 7 : MODEL == kKb4 ? 8 : MODEL == kRational6 ? 10 : 4;
  constexpr bool kThreeCols = (7 + nk) <= 12;
  constexpr bool kSideGrad = nk >= 10;         // 16 Jacobian columns: J^T r is accumulated beside the matrix pipe (kGGrad)
  const int off = cnt_in >= 0 ? off_in : __builtin_amdgcn_readfirstlane(v.tile_off[tile]);
  const int cnt = cnt_in >= 0 ? cnt_in : __builtin_amdgcn_readfirstlane(v.tile_off[tile + 1]) - off;
  const int b = (lane >> 2) & 3, i4 = lane & 3;
  // column-block patterns of the three operand reads
  const int xa = b;
  const int xb = kThreeCols ? (b == 0 ? 0 : b == 1 ? 0 : b == 2 ? 1 : 3) : ((b + 1) & 3);
  const int xc = kThreeCols ? (b == 0 ? 1 : b == 1 ? 2 : b == 2 ? 2 : 3) : ((b + 2) & 3);
  double acc[2][3] = {{0.0, 0.0, 0.0}, {0.0, 0.0, 0.0}};
  double cost = 0.0;
  double gacc[kSideGrad ? 16 : 1];
#pragma unroll
  for (int i = 0; i < (kSideGrad ? 16 : 1); ++i) gacc[i] = 0.0;
#ifdef VC_JAC_STAMPS
#define JSTAMP(i) do { if (tile == 0 && lane == 0) v.dbg[8 + (i)] = (long long)__builtin_readcyclecounter(); } while (0)
#else
#define JSTAMP(i) do {} while (0)
#endif
  JSTAMP(0);
  if (cnt > 0) {
    TileXf x;
    make_tile_xf(pose, cam, &x);
    double K[nk > 8 ? nk : 8];
#pragma unroll
    for (int i = 0; i < (nk > 8 ? nk : 8); ++i) K[i] = cam[kCamK + i];
    ModelPre pre;
    model_precompute(MODEL, K, &pre);
    double* mine = wl + lane * kDotStride;
    // row (lane >> 4) of a 4-row group: corner (lane >> 5), residual row (lane >> 4) & 1
    const double* rowp = wl + (lane >> 5) * kDotStride + ((lane >> 4) & 1) * 16 + i4;
    const double* pa = rowp + 4 * xa;
    const double* pb = rowp + 4 * xb;
    const double* pc = rowp + 4 * xc;
    // four column blocks: the (b, b + 2) products of TWO steps share one instruction -- blocks 0, 1 take them from the even step
    // (A = block b, B = block b + 2), blocks 2, 3 from the odd step (A = block b - 2, B = block b); see `pair_step`
    const double* pa2 = rowp + (b < 2 ? 4 * b : 4 * (b - 2) + 2 * kDotStride);
    const double* pb2 = rowp + (b < 2 ? 4 * (b + 2) : 4 * b + 2 * kDotStride);
    // software prefetch: the corner of the NEXT pass (detection + target point) is in flight while this pass computes
    double2 uv_n = make_double2(0.0, 0.0);
    double pw_n[3] = {0.0, 0.0, 0.0};
    int id_n = 0;
    if (lane < cnt) {
      uv_n = v.obs_uv[off + lane];
      id_n = v.obs_pt[off + lane];
      const double* pp = v.points + 3 * (size_t)(id_n & kObsPointMask);
      pw_n[0] = pp[0]; pw_n[1] = pp[1]; pw_n[2] = pp[2];
    }
    for (int base = 0; base < cnt; base += 64) {
      const int d = base + lane;
      const double2 uv = uv_n;
      const double pw[3] = {pw_n[0], pw_n[1], pw_n[2]};
      const double mult_d = (id_n & kObsOneLess) ? mult - 1.0 : mult;
      if (d + 64 < cnt) {
        uv_n = v.obs_uv[off + d + 64];
        id_n = v.obs_pt[off + d + 64];
        const double* pp = v.points + 3 * (size_t)(id_n & kObsPointMask);
        pw_n[0] = pp[0]; pw_n[1] = pp[1]; pw_n[2] = pp[2];
      }
      if (base == 0) JSTAMP(1);
      if (d < cnt) {
        if (kSideGrad) {
          double rs[2];
          cost += corner_rows<MODEL>(x, K, pre, pw, uv.x, uv.y, mult_d, mine, mine + 16, rs);
#pragma unroll
          for (int i = 0; i < (kSideGrad ? 16 : 1); ++i) gacc[i] += mine[i] * rs[0] + mine[16 + i] * rs[1];
        } else {
          cost += corner_rows<MODEL>(x, K, pre, pw, uv.x, uv.y, mult_d, mine, mine + 16);
        }
      } else {
#pragma unroll
        for (int i = 0; i < 32; ++i) mine[i] = 0.0;
      }
      wave_lds_sync();
      if (base == 0) JSTAMP(2);
      const int ngroups = (min(64, cnt - base) + 1) >> 1;      // groups of 4 rows (2 corners) that hold data; the rest is zero
      auto step = [&](int s, double a, double bb, double cc) {      // three column blocks: 2 instructions per step
        acc[s][0] = __builtin_amdgcn_mfma_f64_4x4x4f64(a, a, acc[s][0], 0, 0, 0);
        acc[s][1] = __builtin_amdgcn_mfma_f64_4x4x4f64(bb, cc, acc[s][1], 0, 0, 0);     // A = (0,0,1,3), B = (1,2,2,3)
      };
      // Four column blocks: a step needs the 10 distinct 4x4 blocks of the symmetric 16x16 product -- diagonal (4), (b, b + 1)
      // (4, with (3,0) for (0,3)) and (0,2), (1,3).  The four blocks of an instruction are independent, so the two (b, b + 2)
      // products of two consecutive steps fill ONE instruction: 5 instructions per two steps instead of 6 (the third
      // instruction of a step used to compute (2,0) and (3,1) a second time).  The matrix pipe is what this kernel saturates
      // (profiles/r03_sq_sweep_cfg4_2500.txt), so the instruction count is its time.
      auto pair_step = [&](int s, double a0, double b0, double a1, double b1, double a2, double b2) {
        acc[0][0] = __builtin_amdgcn_mfma_f64_4x4x4f64(a0, a0, acc[0][0], 0, 0, 0);
        acc[0][1] = __builtin_amdgcn_mfma_f64_4x4x4f64(a0, b0, acc[0][1], 0, 0, 0);
        acc[1][0] = __builtin_amdgcn_mfma_f64_4x4x4f64(a1, a1, acc[1][0], 0, 0, 0);
        acc[1][1] = __builtin_amdgcn_mfma_f64_4x4x4f64(a1, b1, acc[1][1], 0, 0, 0);
        acc[s][2] = __builtin_amdgcn_mfma_f64_4x4x4f64(a2, b2, acc[s][2], 0, 0, 0);
      };
      if (kThreeCols) {
        if (ngroups == 32) {
          // full pass, straight-line: operands of 4 groups at a time, the next chunk's LDS reads in flight under the
          // current chunk's MFMAs
          double ua[2][4], ub[2][4], uc[2][4];
#pragma unroll
          for (int g = 0; g < 4; ++g) { ua[0][g] = pa[g * 2 * kDotStride]; ub[0][g] = pb[g * 2 * kDotStride]; uc[0][g] = pc[g * 2 * kDotStride]; }
#pragma unroll
          for (int c = 0; c < 8; ++c) {
            if (c < 7) {
#pragma unroll
              for (int g = 0; g < 4; ++g) {
                const int gg = (c + 1) * 4 + g;
                ua[(c + 1) & 1][g] = pa[gg * 2 * kDotStride]; ub[(c + 1) & 1][g] = pb[gg * 2 * kDotStride]; uc[(c + 1) & 1][g] = pc[gg * 2 * kDotStride];
              }
            }
#pragma unroll
            for (int g = 0; g < 4; ++g) step(g & 1, ua[c & 1][g], ub[c & 1][g], uc[c & 1][g]);
          }
        } else {
          // ragged last pass: chunks of 8 groups (rows past the data are zero, so a chunk may run over the end)
          for (int g0 = 0; g0 < ngroups; g0 += 8) {
            double va[8], vb[8], vc8[8];
#pragma unroll
            for (int g = 0; g < 8; ++g) { va[g] = pa[(g0 + g) * 2 * kDotStride]; vb[g] = pb[(g0 + g) * 2 * kDotStride]; vc8[g] = pc[(g0 + g) * 2 * kDotStride]; }
#pragma unroll
            for (int g = 0; g < 8; ++g) step(g & 1, va[g], vb[g], vc8[g]);
          }
        }
      } else {
        if (ngroups == 32) {
          // full pass, straight-line: two pairs of steps at a time, the next chunk's LDS reads in flight under the MFMAs
          double ua[2][4], ub[2][4], u2a[2][2], u2b[2][2];
#pragma unroll
          for (int g = 0; g < 4; ++g) { ua[0][g] = pa[g * 2 * kDotStride]; ub[0][g] = pb[g * 2 * kDotStride]; }
#pragma unroll
          for (int q = 0; q < 2; ++q) { u2a[0][q] = pa2[q * 4 * kDotStride]; u2b[0][q] = pb2[q * 4 * kDotStride]; }
#pragma unroll
          for (int c = 0; c < 8; ++c) {
            if (c < 7) {
#pragma unroll
              for (int g = 0; g < 4; ++g) {
                const int gg = (c + 1) * 4 + g;
                ua[(c + 1) & 1][g] = pa[gg * 2 * kDotStride]; ub[(c + 1) & 1][g] = pb[gg * 2 * kDotStride];
              }
#pragma unroll
              for (int q = 0; q < 2; ++q) {
                const int pp = (c + 1) * 2 + q;
                u2a[(c + 1) & 1][q] = pa2[pp * 4 * kDotStride]; u2b[(c + 1) & 1][q] = pb2[pp * 4 * kDotStride];
              }
            }
#pragma unroll
            for (int q = 0; q < 2; ++q)
              pair_step(q, ua[c & 1][2 * q], ub[c & 1][2 * q], ua[c & 1][2 * q + 1], ub[c & 1][2 * q + 1], u2a[c & 1][q], u2b[c & 1][q]);
          }
        } else {
          // ragged last pass: chunks of 4 pairs of steps (rows past the data are zero, so a chunk may run over the end)
          for (int g0 = 0; g0 < ngroups; g0 += 8) {
            double va[8], vb[8], v2a[4], v2b[4];
#pragma unroll
            for (int g = 0; g < 8; ++g) { va[g] = pa[(g0 + g) * 2 * kDotStride]; vb[g] = pb[(g0 + g) * 2 * kDotStride]; }
#pragma unroll
            for (int q = 0; q < 4; ++q) { v2a[q] = pa2[(g0 / 2 + q) * 4 * kDotStride]; v2b[q] = pb2[(g0 / 2 + q) * 4 * kDotStride]; }
#pragma unroll
            for (int q = 0; q < 4; ++q) pair_step(q & 1, va[2 * q], vb[2 * q], va[2 * q + 1], vb[2 * q + 1], v2a[q], v2b[q]);
          }
        }
      }
      wave_lds_sync();
      if (base == 0) JSTAMP(3);
    }
  }
  JSTAMP(4);
  // D lane = 16 i + 4 b + j holds G[4 I_b + i][4 J_b + j]; the packed record takes the upper triangle only (unused blocks stay zero
  // from upload)
  {
    const int i = lane >> 4, j = lane & 3;
    const double d0 = acc[0][0] + acc[1][0], d1 = acc[0][1] + acc[1][1], d2 = acc[0][2] + acc[1][2];
    const int r0 = 4 * b + i, c0 = 4 * b + j;
    if (i <= j) G[g_pack_idx(r0, c0)] = d0;
    const int r1 = 4 * (kThreeCols ? xb : b) + i, c1 = 4 * (kThreeCols ? xc : ((b + 1) & 3)) + j;
    G[g_pack_idx(r1, c1)] = d1;                      // (an off-diagonal block: g_pack_idx orders the pair)
    if (!kThreeCols) {
      // blocks 2, 3 hold the odd steps' share of (0,2), (1,3): added to blocks 0, 1 (eight lanes further on in the row of 16)
      const double d2o = dpp_row_f64<0x128, 0xF>(d2, d2);      // row_ror:8
      if (b < 2) {
        const double d2t = d2 + d2o;
        const int r2 = 4 * b + i, c2 = 4 * (b + 2) + j;
        G[g_pack_idx(r2, c2)] = d2t;
      }
    }
  }
  if (kSideGrad) {
#pragma unroll
    for (int i = 0; i < (kSideGrad ? 16 : 1); ++i) {
      const double t = wave_sum(gacc[i]);
      if (lane == 0) G[kGPackGrad + i] = t;
    }
  }
  JSTAMP(5);
  return wave_sum(cost);          // valid in lane 0
}
// ---- fov / linear / poly2 / poly3 (round 6): the two residual rows of a corner have DIFFERENT structural zeros ------------------------------
// Row u of a radial model has no entry in the columns of fy and cy, row v none in fx and cx: of the 11 .. 14 used columns of
// [A | A x q | B | r] each row type fills 9 .. 12 -- THREE block columns of four (poly2 / poly3: instead of four; fov / linear: three
// before as well, but with both row types in every k-step: 16 sub-block slots per four corners for 12 products).  The Gram block is the sum of the two row
// types' Gram blocks, G = sum u_row^T u_row + sum v_row^T v_row, each over its own compact columns (6 sub-blocks of 4 x 4 instead of 10):
// a group of four corners costs THREE v_mfma_f64_4x4x4 (12 sub-block slots, all used: u-type rows of the four corners as the k dimension
// for six of them, v-type rows for the other six) where the four-block-column form needs five for the same four corners (two k-steps of two
// corners x two rows).  The matrix instructions are this kernel's time: -40 % of them for these models.  The two compact
// 12 x 12 blocks are added into the packed 16 x 16 record once per tile.
//   compact column j of row type t:  0..5 -> A, A x q;  6 -> fx | fy;  7 -> cx | cy;  8.. -> the nk - 4 distortion terms;  then r
template <int MODEL>
__device__ __forceinline__ double jac_tile_body_split(const DevView& v, const double* pose, const double* cam, double mult, int tile, int lane,
                                                      double* wl, double* G, int off_in, int cnt_in) {
  static_assert(MODEL == kPoly2 || MODEL == kPoly3 || MODEL == kFov || MODEL == kLinear, "split rows: the radial models with at most seven intrinsics");
  constexpr int nk = MODEL == kFov ? 5 : MODEL == kPoly2 ? 6 : MODEL == kPoly3 ? 7 : 4;
  constexpr int nd = nk - 4;                       // distortion terms
  constexpr int ncomp = 9 + nd;                    // compact columns in use (11 / 12)
  const int off = cnt_in >= 0 ? off_in : __builtin_amdgcn_readfirstlane(v.tile_off[tile]);
  const int cnt = cnt_in >= 0 ? cnt_in : __builtin_amdgcn_readfirstlane(v.tile_off[tile + 1]) - off;
  const int b = (lane >> 2) & 3, i4 = lane & 3, kq = lane >> 4;
  // (row type, block column of A, of B) of block b in the three instructions of a group
  const int t0 = b == 3 ? 1 : 0, xa0 = b == 3 ? 0 : b, xb0 = xa0;                                   // (0;0,0) (0;1,1) (0;2,2) (1;0,0)
  const int t1 = b == 3 ? 1 : 0, xa1 = b == 0 ? 0 : b == 1 ? 0 : 1, xb1 = b == 0 ? 1 : b == 1 ? 2 : b == 2 ? 2 : 1;      // (0;0,1) (0;0,2) (0;1,2) (1;1,1)
  const int xa2 = b == 0 ? 2 : b == 1 ? 0 : b == 2 ? 0 : 1, xb2 = b == 0 ? 2 : b == 1 ? 1 : 2;      // (1;2,2) (1;0,1) (1;0,2) (1;1,2)
  double acc[2][3] = {{0.0, 0.0, 0.0}, {0.0, 0.0, 0.0}};
  double cost = 0.0;
  if (cnt > 0) {
    TileXf x;
    make_tile_xf(pose, cam, &x);
    double K[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) K[i] = cam[kCamK + i];
    ModelPre pre;
    model_precompute(MODEL, K, &pre);
    double* mine = wl + lane * kDotStride;
    const double* rowp = wl + kq * kDotStride + i4;                    // row kq of a group of four corners
    const double* pa0 = rowp + t0 * 16 + 4 * xa0; const double* pb0 = rowp + t0 * 16 + 4 * xb0;
    const double* pa1 = rowp + t1 * 16 + 4 * xa1; const double* pb1 = rowp + t1 * 16 + 4 * xb1;
    const double* pa2 = rowp + 16 + 4 * xa2;      const double* pb2 = rowp + 16 + 4 * xb2;
    double2 uv_n = make_double2(0.0, 0.0);
    double pw_n[3] = {0.0, 0.0, 0.0};
    int id_n = 0;
    if (lane < cnt) {
      uv_n = v.obs_uv[off + lane];
      id_n = v.obs_pt[off + lane];
      const double* pp = v.points + 3 * (size_t)(id_n & kObsPointMask);
      pw_n[0] = pp[0]; pw_n[1] = pp[1]; pw_n[2] = pp[2];
    }
    for (int base = 0; base < cnt; base += 64) {
      const int d = base + lane;
      const double2 uv = uv_n;
      const double pw[3] = {pw_n[0], pw_n[1], pw_n[2]};
      const double mult_d = (id_n & kObsOneLess) ? mult - 1.0 : mult;
      if (d + 64 < cnt) {
        uv_n = v.obs_uv[off + d + 64];
        id_n = v.obs_pt[off + d + 64];
        const double* pp = v.points + 3 * (size_t)(id_n & kObsPointMask);
        pw_n[0] = pp[0]; pw_n[1] = pp[1]; pw_n[2] = pp[2];
      }
      if (d < cnt) {
        double r0[16], r1[16];
        cost += corner_rows<MODEL>(x, K, pre, pw, uv.x, uv.y, mult_d, r0, r1);
        // compact rows: u drops fy (7), cy (9); v drops fx (6), cx (8)
#pragma unroll
        for (int j = 0; j < 6; ++j) { mine[j] = r0[j]; mine[16 + j] = r1[j]; }
        mine[6] = r0[6]; mine[7] = r0[8]; mine[16 + 6] = r1[7]; mine[16 + 7] = r1[9];
#pragma unroll
        for (int j = 0; j < nd + 1; ++j) { mine[8 + j] = r0[10 + j]; mine[16 + 8 + j] = r1[10 + j]; }      // distortion terms, then the residual (column 6 + nk)
#pragma unroll
        for (int j = ncomp; j < 12; ++j) { mine[j] = 0.0; mine[16 + j] = 0.0; }
      } else {
#pragma unroll
        for (int i = 0; i < 12; ++i) { mine[i] = 0.0; mine[16 + i] = 0.0; }
      }
      wave_lds_sync();
      const int ngroups = (min(64, cnt - base) + 3) >> 2;      // groups of four corners that hold data; rows past the data are zero
      auto fetch = [&](int g, double* a3, double* b3) {
        const int o = g * 4 * kDotStride;
        a3[0] = pa0[o]; b3[0] = pb0[o]; a3[1] = pa1[o]; b3[1] = pb1[o]; a3[2] = pa2[o]; b3[2] = pb2[o];
      };
      if (ngroups == 16) {
        // full pass, straight-line: operands of four groups at a time, the next chunk's LDS reads in flight under the current chunk's MFMAs
        double ua[2][4][3], ub[2][4][3];
#pragma unroll
        for (int g = 0; g < 4; ++g) fetch(g, ua[0][g], ub[0][g]);
#pragma unroll
        for (int c = 0; c < 4; ++c) {
          if (c < 3) {
#pragma unroll
            for (int g = 0; g < 4; ++g) fetch((c + 1) * 4 + g, ua[(c + 1) & 1][g], ub[(c + 1) & 1][g]);
          }
#pragma unroll
          for (int g = 0; g < 4; ++g)
#pragma unroll
            for (int n = 0; n < 3; ++n) acc[g & 1][n] = __builtin_amdgcn_mfma_f64_4x4x4f64(ua[c & 1][g][n], ub[c & 1][g][n], acc[g & 1][n], 0, 0, 0);
        }
      } else {
        for (int g0 = 0; g0 < ngroups; g0 += 4) {              // ragged last pass: chunks of four groups (a chunk may run over the end into zero rows)
          double ua[4][3], ub[4][3];
#pragma unroll
          for (int g = 0; g < 4; ++g) fetch(g0 + g, ua[g], ub[g]);
#pragma unroll
          for (int g = 0; g < 4; ++g)
#pragma unroll
            for (int n = 0; n < 3; ++n) acc[g & 1][n] = __builtin_amdgcn_mfma_f64_4x4x4f64(ua[g][n], ub[g][n], acc[g & 1][n], 0, 0, 0);
        }
      }
      wave_lds_sync();
    }
  }
  // ---- the two compact blocks -> the packed record.  D lane = 16 i + 4 b + j holds entry (4 XA + i, 4 XB + j) of row type t's block.
  {
    double* GC = wl;                                // [2][12 x 12], upper block triangle written (this wavefront's corner rows are done with)
    const int i = lane >> 4, j = lane & 3;
    const double d0 = acc[0][0] + acc[1][0], d1 = acc[0][1] + acc[1][1], d2 = acc[0][2] + acc[1][2];
    GC[t0 * 144 + (4 * xa0 + i) * 12 + 4 * xb0 + j] = d0;
    GC[t1 * 144 + (4 * xa1 + i) * 12 + 4 * xb1 + j] = d1;
    GC[144 + (4 * xa2 + i) * 12 + 4 * xb2 + j] = d2;
    wave_lds_sync();
    // compact column of full column fc in row type t (-1: structurally zero there / unused)
    auto comp = [&](int fc, int t) {
      return fc < 6 ? fc : fc == 6 ? (t == 0 ? 6 : -1) : fc == 7 ? (t == 1 ? 6 : -1) : fc == 8 ? (t == 0 ? 7 : -1) : fc == 9 ? (t == 1 ? 7 : -1)
           : fc <= 6 + nk ? 8 + (fc - 10) : -1;
    };
#pragma unroll
    for (int q = 0; q < 3; ++q) {
      const int e = lane + 64 * q;
      if (e < kGPackGrad) {
        int r = 0;
#pragma unroll
        for (int a2 = 1; a2 < 16; ++a2) r += (e >= a2 * 16 - (a2 * (a2 - 1)) / 2) ? 1 : 0;      // row of packed entry e
        const int c = r + (e - (r * 16 - (r * (r - 1)) / 2));
        double s = 0.0;
#pragma unroll
        for (int t = 0; t < 2; ++t) {
          const int jr = comp(r, t), jc = comp(c, t);
          // (the upper block triangle is what was written: entry (jr, jc), jr <= jc, lies in block (jr / 4, jc / 4); inside a diagonal
          //  block both triangles are there)
          const double g = GC[t * 144 + (jr >= 0 ? jr : 0) * 12 + (jc >= 0 ? jc : 0)];
          s += (jr >= 0 && jc >= 0) ? g : 0.0;
        }
        G[e] = s;
      }
    }
  }
  return wave_sum(cost);          // valid in lane 0
}
__device__ __forceinline__ double jac_tile_dispatch(const DevView& v, int model, const double* pose, const double* cam, double mult, int tile,
                                                    int lane, double* wl, double* G, int off = 0, int cnt = -1) {
  switch (model) {   // wave-uniform
    case kFov: return jac_tile_body<kFov>(v, pose, cam, mult, tile, lane, wl, G, off, cnt);
    // (fov / linear through the split form as well -- 48 instead of 64 matrix instructions per pass -- measured SLOWER: 237 against 233.5 us
    //  at cfg5 / 6250 frames, k_trial 16.8 against 15.6 us at cfg2: their tiles are three passes long and the per-tile assembly of the
    //  two compact blocks costs more than the instructions saved; poly3 at cfg4's nine passes per tile: 150 against 161 us)
    case kPoly2: return jac_tile_body_split<kPoly2>(v, pose, cam, mult, tile, lane, wl, G, off, cnt);
    case kPoly3: return jac_tile_body_split<kPoly3>(v, pose, cam, mult, tile, lane, wl, G, off, cnt);
    case kKb4: return jac_tile_body<kKb4>(v, pose, cam, mult, tile, lane, wl, G, off, cnt);
    case kRational6: return jac_tile_body<kRational6>(v, pose, cam, mult, tile, lane, wl, G, off, cnt);
    default: return jac_tile_body<kLinear>(v, pose, cam, mult, tile, lane, wl, G, off, cnt);
  }
}

// trial = 0: linearisation at the accepted state (only when the control record asks for one); trial = 1: the sweep runs at the
// trial state and fills buffer 1 - cur -- its cost is the trial cost, its Gram blocks are the next linearisation if the step is
// accepted (the decision flips `cur`), and a rejected step leaves buffer cur untouched.
#ifndef VC_JAC_WAVES
#define VC_JAC_WAVES 2
#endif
__global__ __launch_bounds__(256, VC_JAC_WAVES) void k_reproj_jac(DevView v, int trial) {
  extern __shared__ __attribute__((aligned(16))) double lds[];
  const Ctrl* ct = v.ctrl;
#ifdef VC_JAC_STAMPS
  if (blockIdx.x == 0 && threadIdx.x == 0) v.dbg[7] = (long long)__builtin_readcyclecounter();
#endif
  __shared__ double s_cost[4];
  // the trial sweep follows the back-substitution on the main stream: that this kernel has started says the trial poses are complete
  // and written back -- published for the second stream's k_imu_jac (no event record between the two kernels of the critical path)
  if (trial && blockIdx.x == 0 && threadIdx.x == 0) signal_started(v, 2);
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int tile = blockIdx.x * 4 + wave;
  // the tile's header (frame, camera, model, corner range: one 48-byte record) is requested together with the control record, not behind
  // it (round 6: control record -> tile_frame / tile_cam -> model -> tile_off -> corners -> target points were five dependent round
  // trips at the head of a 17 us kernel; now three)
  const TileHdr h = v.tile_hdr[tile < v.n_tiles ? tile : 0];
  const int c_done = ct->done, c_need = ct->need_lin, c_cur = ct->cur;
  const double c_mult = ct->mult;
  if (c_done || (!trial && !c_need)) return;
  double cost = 0.0;
  if (tile < v.n_tiles) {
    double* wl = lds + wave * 64 * kDotStride;
    const int cur = trial ? 1 - c_cur : c_cur;
    const int f = __builtin_amdgcn_readfirstlane(h.frame), c = __builtin_amdgcn_readfirstlane(h.cam);
    cost = jac_tile_dispatch(v, __builtin_amdgcn_readfirstlane(h.model), v.poses[cur] + (size_t)f * kPoseStride, v.cams[cur] + (size_t)c * kCamStride, c_mult,
                             tile, lane, wl, v.Gb[cur] + (size_t)tile * kGPack, __builtin_amdgcn_readfirstlane(h.off), __builtin_amdgcn_readfirstlane(h.cnt));
    if (lane == 0) v.tile_costb[cur][tile] = cost;
  }
  if (trial) {               // the workgroup's share of the trial cost, in fixed order
    if (lane == 0) s_cost[wave] = cost;
    __syncthreads();
    if (threadIdx.x == 0) v.wg_trial[blockIdx.x] = (s_cost[0] + s_cost[1]) + (s_cost[2] + s_cost[3]);
  }
}

}  // namespace vc
