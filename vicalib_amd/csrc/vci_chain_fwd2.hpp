// vci_chain_fwd2.hpp -- chain_eliminate, k_chain_fwd2: one level of the chain elimination from both ends of every group at once.
// Kernel fragment of vc_imu_kernels.hip alone (defines __global__ symbols; included there in stage order; not for host harnesses).
#pragma once
#include <hip/hip_runtime.h>
#include "vc_math.hpp"
#include "vc_device.h"
#include "vc_kutil.hpp"
#include "vc_shared_blocks.hpp"
#include "vci_chain_fwd.hpp"

namespace vc {

// ---- one elimination of a two-sided sweep (k_chain_fwd2, k_chain_l0) --------------------------------------------------------------------
// The frame's block A is in An (LDS, complete behind the first synchronisation); lane = image column, x = the lane's column of the
// frame's image (role: 0 border (W | g), 1 C, 2 A, 3 B, 4 none; sub = column inside the 9 x 9 block; pc = the column's position in an
// image row).  A = L L^T in EVERY lane, from registers (round 4; before: nine lanes, one row each, pivots and pivot columns through
// v_readlane -- ~240 cycles per pivot, 0.9 us per frame, and the factor went through LDS to the lanes that solve with it): all lanes
// read the lower triangle (broadcast LDS reads) and run the same scalar factorisation -- per pivot one v_rsq_f64 chain, then independent
// multiplies / FMAs; the triangular solve that follows takes L from registers.  The solved column goes to the frame's image
// [Y | z | X_s | L | X_n] in HBM, [X_s | X_n] to XS (LDS) for everybody, out = [X_s | X_n]^T (column).
// WG_SYNC: the sweep is several wavefronts side by side (k_chain_fwd2<NW > 1>): workgroup barriers instead of wavefront-local ones.
// a double at a BYTE offset from a wave-uniform base: scalar base + 32-bit lane offset (global_load / global_store with an SGPR pair as the
// address and one VGPR as the offset) instead of a 64-bit address per lane and access.  A lone wavefront pays ~4 cycles for EVERY instruction
// it issues, address arithmetic included: per frame of a two-sided sweep the columns' addresses were ~340 instructions, the frame's
// elimination itself ~850 (round 6, tools/isa_classes.py with markers).  Images stay below 4 GB (n_frames x 9 x ldx x 8: 0.9 GB at 50 000 frames).
__device__ __forceinline__ double ld_boff(const double* base, unsigned boff) { return *reinterpret_cast<const double*>(reinterpret_cast<const char*>(base) + boff); }
struct ElimLds { double* XS; double* An; double* Ls; };
template <bool WG_SYNC>
__device__ __forceinline__ void chain_eliminate(const DevView& v, double* img /* the frame's image */, int ldx, int role, int pc, int sub, bool flag_lane,
                                                const ElimLds& M, double* x, double* out, long long* stamp = nullptr /* profiling builds: phase stamps of this call */) {
  auto gsync = [&]() { if (WG_SYNC) __syncthreads(); else wave_lds_sync_local(); };
#ifdef VC_F2_STAMPS
#define ELSTAMP(i) do { if (stamp) stamp[i] = (long long)__builtin_amdgcn_s_memrealtime(); } while (0)
#else
#define ELSTAMP(i) do { } while (0)
#endif
  double* XS = M.XS; double* An = M.An; double* Ls = M.Ls;
  ELSTAMP(0);
  gsync();
  ELSTAMP(1);
  double Lr[45], dinv[9];
  {
#pragma unroll
    for (int i = 0; i < 9; ++i)
#pragma unroll
      for (int j = 0; j <= i; ++j) Lr[i * (i + 1) / 2 + j] = An[i * 9 + j];
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
      for (int i = j + 1; i < 9; ++i) Lr[i * (i + 1) / 2 + j] *= ip;
#pragma unroll
      for (int i = j + 1; i < 9; ++i)
#pragma unroll
        for (int k = j + 1; k <= i; ++k) Lr[i * (i + 1) / 2 + k] -= Lr[i * (i + 1) / 2 + j] * Lr[k * (k + 1) / 2 + j];
    }
    if (bad) {               // wave-uniform (every lane holds the same numbers): the frame gets an identity block, the pass is flagged
      if (flag_lane) atomicAdd(&v.flags[4 + 2 * v.par], 1);
#pragma unroll
      for (int i = 0; i < 9; ++i) {
        dinv[i] = 1.0;
#pragma unroll
        for (int j = 0; j <= i; ++j) Lr[i * (i + 1) / 2 + j] = (i == j) ? 1.0 : 0.0;
      }
    }
  }
  ELSTAMP(2);
#pragma unroll
  for (int k = 0; k < 9; ++k) {
    x[k] *= dinv[k];
#pragma unroll
    for (int rr = k + 1; rr < 9; ++rr) x[rr] -= Lr[rr * (rr + 1) / 2 + k] * x[k];
  }
  ELSTAMP(3);
  // Hand-over through LDS, WITHOUT a divergent branch per role (round 6: the five `if (role == ..)` regions of this function were ~40 exec-mask
  // and branch instructions per elimination of a wavefront that is alone on its SIMD and pays ~4 cycles for every instruction it issues):
  // every lane stores its nine values through ONE address pattern chosen by its role --
  //   A lanes: row `sub` of L (x = L^T e_sub) as column `sub` of Ls (the image wants the column: the nine lanes transpose here),
  //   C / B lanes: their solved column into [X_s | X_n],   everybody else: the padding column 18 of XS (never read).
  {
    double* dst = role == 2 ? Ls + sub : XS + (role == 1 ? sub : role == 3 ? 9 + sub : 18);
    const int st = role == 2 ? 9 : kXsLd;
#pragma unroll
    for (int k = 0; k < 9; ++k) dst[k * st] = (role == 2 && k > sub) ? 0.0 : x[k];
  }
  ELSTAMP(4);
  gsync();
  ELSTAMP(5);
  // the frame's solved image [Y | z | X_s | L | X_n]: one store region for all lanes that own a column; the A lanes store L's column and
  // carry on with X_n's column `sub` (the A columns of the next frame are driven by X_n's)
  {
    const double* rl = Ls + (role == 2 ? sub * 9 : 0);
    const double* rx = XS + (role == 2 ? 9 + sub : 18);
    double lv[9], xv[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) { lv[k] = rl[k]; xv[k] = rx[k * kXsLd]; }
    if (role < 4) {
      // (a 64-bit address per lane: storing through a scalar base + byte offsets as the loads do was slower -- same-box A/B: the folded
      //  bottom level 28.0 -> 30.0 us, the upper levels unchanged)
      double* ic = img + pc;
#pragma unroll
      for (int k = 0; k < 9; ++k) ic[k * ldx] = role == 2 ? lv[k] : x[k];       // (A: L[k][sub], zero above the diagonal)
    }
#pragma unroll
    for (int k = 0; k < 9; ++k) x[k] = role == 2 ? xv[k] : x[k];
  }
  ELSTAMP(6);
  // out = [X_s | X_n]^T x in two halves: rows 9..17 (the next frame's update, which the critical path waits for) first
#pragma unroll
  for (int h = 1; h >= 0; --h) {
#pragma unroll
    for (int rr = 0; rr < 9; ++rr) out[9 * h + rr] = 0.0;
#pragma unroll
    for (int k = 0; k < 9; ++k) {
      const double xk = x[k];
#pragma unroll
      for (int rr = 0; rr < 9; ++rr) out[9 * h + rr] += XS[k * kXsLd + 9 * h + rr] * xk;
    }
    if (h == 1) __builtin_amdgcn_sched_barrier(0);
  }
  ELSTAMP(7);
}

// ---- two-sided elimination of a group (narrow borders: one column per lane) ------------------------------------------------
// A full group [a | e_1 .. e_{m-1} | r] is eliminated from both ends at once: wavefront 0 sweeps e_1, e_2, .. left to right
// against the left separator a (exactly the one-sided scheme), wavefront 1 sweeps e_{m-1}, e_{m-2}, .. right to left against the
// right separator r -- the same recurrence on the mirrored chain: its "coupling to the next frame" is the transposed B block of the
// frame to its left, its first frame's coupling to the separator is that frame's own B block, its separator updates go to r's side
// image -- and the middle frame, which receives the updates of both sweeps, is eliminated last by wavefront 0 with a on one side and
// r on the other.  (m - 2) / 2 + 1 dependent eliminations per level instead of m - 1: 4 instead of 7 at m = 8.  Needs m >= 4.
// Images of the right sweep's frames hold [Y | z | X_s (coupling to r) | L | X_n (coupling to the frame on the LEFT)]; the
// back-substitution (k_chain_back, two = 1) mirrors the order.  The short group at the chain's end works the same way without r.
#ifdef VC_F2_STAMPS
#define F2STAMP(i) do { if (NW == 1 && blockIdx.x == 0 && lvl == 1 && threadIdx.x == 0 && (i) < 16) v.dbg[(i)] = (long long)__builtin_amdgcn_s_memrealtime(); } while (0)      // (sweep 0; dbg[16..23]: the phases of its second elimination, chain_eliminate)
#else
#define F2STAMP(i) do { } while (0)
#endif
// NW > 1 (round 4): borders wider than one column per lane -- every sweep is NW wavefronts side by side (column c = lane + 64 u, as in
// chain_fwd_group), the group a workgroup of 2 NW wavefronts; the exchanges inside a sweep go through workgroup barriers, which both
// sweeps then meet in lockstep (a sweep with one frame less runs an empty round).  ~370 registers: one wavefront per SIMD, so NW = 2 fills
// a CU -- used on levels whose groups the chip holds at once (chain_levels).
template <int NW>
#ifndef VC_FWD2_WAVES
#define VC_FWD2_WAVES 1
#endif
__global__ __launch_bounds__(128 * NW, VC_FWD2_WAVES) void k_chain_fwd2(DevView v, int s, int m, int lvl, int n_groups) {
  constexpr int W = 64 * NW;
  __shared__ __attribute__((aligned(16))) double XS2[2][9 * kXsLd];
  __shared__ double An2[2][81], Ls2[2][81];
  __shared__ double MID[9 * W];      // right sweep -> wavefront 0: its update of the middle frame (W, A columns) and the middle's coupling to r
  __shared__ double SEPR[9 * W];     // the right sweep's accumulated update of r
  // (round 6) workgroups behind the level's groups: a side job -- the chunk records' camera / IMU / cost entries summed into part_total while
  // the level leaves most of the chip idle (vc_shared_blocks.hpp; DevView::hadd_early)
  if ((int)blockIdx.x >= n_groups) { part_tail_sum_job(v, (int)blockIdx.x - n_groups, MID, 128 * NW); return; }
  // (the wavefront's index as a scalar: everything that depends on it -- sweep direction, frame count, addresses -- stays uniform)
  const int wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), wave = wv / NW /* the sweep */, lane = threadIdx.x & 63, group = blockIdx.x;
  auto gsync = [&]() { if (NW > 1) __syncthreads(); else wave_lds_sync_local(); };
  const int N = v.n_frames, D = v.D, ldw = v.ldw, ldx = v.ldx, nW = D + 1, ncol = nW + 27;
#ifdef VC_F2_STAMPS
  const long long f2_t0 = (long long)__builtin_amdgcn_s_memrealtime();
#endif
  const long gs = (long)m * s;
  const int a = (int)((long)group * gs), first = a + s;
  const int done = v.ctrl->done;
  if (lvl == 1 && blockIdx.x == 0 && threadIdx.x == 0) signal_started(v, 7);      // the bottom level is complete: this launch runs (the weight update waits for it)
  const bool pend = lvl > 0;
  const double* rp = v.rX[(lvl + 1) & 1];
  double* rw = v.rX[lvl & 1];
  const size_t isz = (size_t)9 * ldx;
  const int c = lane + 64 * (wv % NW), e0 = c - nW;
  const int role = c < nW ? 0 : (e0 < 9 ? 1 : e0 < 18 ? 2 : e0 < 27 ? 3 : 4);     // 0 border (W | g), 1 C, 2 A, 3 B, 4 none
  const int pc = c < nW ? c : (c < ncol ? ldw + e0 : 0);
  const int sub = e0 < 9 ? e0 : e0 < 18 ? e0 - 9 : e0 - 18;
  if (first >= N) {            // a separator without interior frames: only its pending right contribution is folded in
    if (!done && wave == 0 && a < N) {
      double* img = v.cW + (size_t)a * isz + pc;
      if ((role == 0 || role == 2) && pend && a > 0) {
#pragma unroll
        for (int k = 0; k < 9; ++k) img[k * ldx] += rp[(size_t)(a / s) * isz + k * ldx + pc];
      } else if (role == 3) {
#pragma unroll
        for (int k = 0; k < 9; ++k) img[k * ldx] = 0.0;
      }
    }
    return;
  }
  const int q = min(m - 1, (N - 1 - first) / s + 1);          // interior frames e_1 .. e_q; the last group of a level may be short
  const int r = first + q * s;                                // right separator, if the chain goes on
  const bool has_r = q == m - 1 && r < N;
  const int nl = (q - 1) / 2, mid = nl + 1, nr = q - 1 - nl;                     // interior indices 1 .. nl | mid | mid + 1 .. q
  const int dir = wave == 0 ? 1 : -1, cnt = wave == 0 ? nl : nr, i0 = wave == 0 ? 1 : q;
  double* XS = XS2[wave]; double* An = An2[wave]; double* Ls = Ls2[wave];
  // the image columns of frame e as this sweep needs them: own values + the pending right contribution of the level below for the
  // border and A; the coupling to the sweep's separator (first frame only: later frames get it as fill-in); the coupling to the
  // next frame of the sweep
  // (branch-free: every lane reads nine values from ONE address pattern -- base + k stride -- chosen by its role, idle lanes read
  // column 0 of the image and scale it by zero; the pending contribution likewise)
  // (round 6: ONE byte offset pattern per lane -- first column entry c0b, step stb -- relative to the image of the frame the lane reads
  //  from (fsel: the sweep's frame e, the left separator a, or the frame e - s whose B block row is this frame's coupling), wave-uniform
  //  bases: 18 offset additions and 18 loads per frame where the 64-bit addresses per lane and load were ~340 instructions)
  const unsigned ldxb = 8u * (unsigned)ldx, iszb = 9u * ldxb;
  unsigned c0b = 0, stb = ldxb; int fsel = 0;
  if (role == 0 || role == 2) c0b = 8u * (unsigned)pc;
  else if (role == 1) { if (dir > 0) { c0b = 8u * (unsigned)(sub * ldx + ldw + 18); stb = 8; fsel = 1; } else c0b = 8u * (unsigned)(ldw + 18 + sub); }
  else if (role == 3) { if (dir > 0) c0b = 8u * (unsigned)pc; else { c0b = 8u * (unsigned)(sub * ldx + ldw + 18); stb = 8; fsel = 2; } }
  const unsigned ab = (unsigned)a * iszb;
  const int qa = group * m;             // e / s of frame e = a + i s is qa + i (a = group m s)
  auto load_cols = [&](int idx /* frame e = a + idx s, idx >= 1 */, bool first_of_sweep, bool with_image, double* x) {
    const int e = a + idx * s;
    const unsigned eb = (unsigned)e * iszb, emb = (unsigned)(e - s) * iszb;
    const unsigned fb = fsel == 1 ? ab : (fsel == 2 ? emb : eb);
    const unsigned pb = (unsigned)(qa + idx) * iszb;      // (the pending image of frame e in rp: one base for the whole kernel, the frame in the offset)
    const bool live0 = with_image && (role == 0 || role == 2 || role == 3 || (role == 1 && first_of_sweep));
    const bool live1 = with_image && pend && (role == 0 || role == 2);
    double y0[9], y1[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) y0[k] = ld_boff(v.cW, fb + c0b + k * stb);
    if (pend) {
#pragma unroll
      for (int k = 0; k < 9; ++k) y1[k] = ld_boff(rp, pb + c0b + k * stb);
    } else {
#pragma unroll
      for (int k = 0; k < 9; ++k) y1[k] = 0.0;
    }
#pragma unroll
    for (int k = 0; k < 9; ++k) x[k] = (live0 ? y0[k] : 0.0) + (live1 ? y1[k] : 0.0);
  };
  double xin[9], o[9], dacc[9];
#pragma unroll
  for (int k = 0; k < 9; ++k) { dacc[k] = 0.0; o[k] = 0.0; }
  // what the left separator will absorb into at the end (its own columns + the right contribution it received one level down):
  // requested now -- nobody else writes them during this level -- so that the kernel ends with stores, not with a load round trip
  double sep0[9];
  {
    const bool pa = pend && a > 0;
    const int pcd = role == 1 ? ldw + 9 + sub : pc;
    const double* img = v.cW + (size_t)a * isz + pcd;
    const double* rpa = rp + (size_t)(a / s) * isz + pcd;
    const bool mine = wave == 0 && (role == 0 || role == 1);
#pragma unroll
    for (int k = 0; k < 9; ++k) sep0[k] = mine ? img[k * ldx] + (pa ? rpa[k * ldx] : 0.0) : 0.0;
  }
  // (a side without frames of its own: wavefront 0 starts with the middle frame, wavefront 1 has nothing to load)
  load_cols(cnt > 0 ? i0 : mid, true, cnt > 0 || wave == 0, xin);
  // (round 6 tried requesting a frame's columns TWO eliminations ahead -- they come from HBM, the level below wrote them from other XCDs --:
  //  21.9 / 21.1 us per level against 20.2 / 19.6: nine more doubles per lane through the accumulation registers cost more than the wait)
  if (done) return;
#ifdef VC_F2_STAMPS
  if (NW == 1 && blockIdx.x == 0 && lvl == 1 && threadIdx.x == 0) v.dbg[0] = f2_t0;
#endif
  F2STAMP(1);
  if (role == 2) {
#pragma unroll
    for (int k = 0; k < 9; ++k) An[k * 9 + sub] = xin[k];
  }
  // one elimination: A (in An) = L L^T, all columns solved, image stored, [X_s | X_n] to XS, out = [X_s | X_n]^T (column)
  const ElimLds elds = {XS, An, Ls};
#ifdef VC_F2_STAMPS
  int el_n_ = 0;
  auto eliminate = [&](int e, double* x, double* out) {
    long long* st = (NW == 1 && blockIdx.x == 0 && lvl == 1 && threadIdx.x == 0 && el_n_ == 1) ? v.dbg + 16 : nullptr;      // (the second elimination of sweep 0)
    ++el_n_;
    chain_eliminate<(NW > 1)>(v, v.cW + (size_t)e * isz, ldx, role, pc, sub, c == 0, elds, x, out, st);
  };
#else
  auto eliminate = [&](int e, double* x, double* out) { chain_eliminate<(NW > 1)>(v, v.cW + (size_t)e * isz, ldx, role, pc, sub, c == 0, elds, x, out); };
#endif
  // The sweep's frames, then -- wavefront 0 only, behind the barrier that hands it the right sweep's results -- the middle frame:
  // a on its left (C), r on its right (B: the right sweep's fill-in, or -- no right sweep -- its own B block, already loaded).
  // One loop, one copy of the elimination: wavefront 1 leaves at the barrier.
  for (int j = 0; ; ++j) {
    const bool at_mid = j == cnt;
    F2STAMP(2 + 2 * j);
    if (at_mid) {
      if (NW > 1) for (int jj = cnt; jj < max(nl, nr); ++jj) { gsync(); gsync(); }      // the other sweep's extra elimination: its barriers
      if (wave == 1) {
        if (cnt == 0) {
#pragma unroll
          for (int k = 0; k < 9; ++k) MID[k * W + c] = 0.0;
        }
#pragma unroll
        for (int k = 0; k < 9; ++k) SEPR[k * W + c] = dacc[k];
      }
      F2STAMP(12);
      __syncthreads();
      F2STAMP(13);
      if (wave == 1) return;
#pragma unroll
      for (int k = 0; k < 9; ++k) {
        if (role == 0 || role == 2) xin[k] += MID[k * W + c];
        else if (role == 3 && nr > 0) xin[k] = MID[k * W + nW + sub];      // (no right sweep: the middle's own B block stays)
      }
      if (role == 2) {
#pragma unroll
        for (int k = 0; k < 9; ++k) An[k * 9 + sub] = xin[k];
      }
    }
    const int e = a + (at_mid ? mid : i0 + dir * j) * s;
    if (!at_mid)                        // the columns of the frame after this one: requested now, used after the elimination
      load_cols(j + 1 < cnt ? i0 + dir * (j + 1) : mid, false, j + 1 < cnt || wave == 0, o);
    double x[9], out[18];
#pragma unroll
    for (int k = 0; k < 9; ++k) x[k] = xin[k];
    eliminate(e, x, out);
    F2STAMP(3 + 2 * j);
#pragma unroll
    for (int k = 0; k < 9; ++k) dacc[k] += out[k];
    if (at_mid) {
      // the right separator's side image: the middle's update and the right sweep's (whose C lanes carry the update of A's columns)
      if (has_r && role < 4) {
        double* ri = rw + (size_t)(r / gs) * isz + pc;
        const bool keep = role == 0 || role == 2;
        const int src = role == 2 ? nW + sub : c;
#pragma unroll
        for (int k = 0; k < 9; ++k) ri[k * ldx] = keep ? -out[9 + k] - SEPR[k * W + src] : 0.0;
      }
      if (role == 3) {                 // the separator's coupling to the right separator at the next level (none where the chain ends)
        double* img = v.cW + (size_t)a * isz + pc;
#pragma unroll
        for (int k = 0; k < 9; ++k) img[k * ldx] = has_r ? -out[k] : 0.0;
      }
      break;
    }
    if (wave == 1 && j + 1 == cnt) {    // the next frame is the middle, which wavefront 0 eliminates: hand the update over
#pragma unroll
      for (int k = 0; k < 9; ++k) MID[k * W + c] = -out[9 + k];
    } else {
#pragma unroll
      for (int k = 0; k < 9; ++k) xin[k] = o[k] - (role == 3 ? 0.0 : out[9 + k]);
      if (role == 2) {
#pragma unroll
        for (int k = 0; k < 9; ++k) An[k * 9 + sub] = xin[k];
      }
    }
  }
  // ---- the left separator absorbs its group (and the right contribution it received one level down)
  if (role == 0 || role == 1) {                      // the C lanes carry the update of A's columns
    const int pcd = role == 1 ? ldw + 9 + sub : pc;
    double* img = v.cW + (size_t)a * isz + pcd;
#pragma unroll
    for (int k = 0; k < 9; ++k) img[k * ldx] = sep0[k] - dacc[k];
  }
  F2STAMP(14);
}

}  // namespace vc
