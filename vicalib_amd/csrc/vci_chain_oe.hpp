// vci_chain_oe.hpp -- chain_oe_group: one level of the elimination by odd-even reduction inside a workgroup of four wavefronts (one-column
// borders, the levels above the bottom one, the top level: vc_chain_order.hpp) -- 3 dependent eliminations per level instead of 4.
// (its kernel k_chain_oe stands behind k_chain_top_gram, the group's other caller, in vc_imu_kernels.hip)
// Fragment of vc_imu_kernels.hip, included there in stage order.
#pragma once
#include <hip/hip_runtime.h>
#include "vc_math.hpp"
#include "vc_device.h"
#include "vc_chain_order.hpp"
#include "vc_kutil.hpp"
#include "vci_chain_fwd2.hpp"

namespace vc {

// ---- odd-even elimination of a group (narrow borders: one column per lane; vc_chain_order.hpp) -------------------------------------------
// The two sweeps of k_chain_fwd2 still leave (m - 2) / 2 + 1 = 4 DEPENDENT eliminations per level, each ~1000 instructions of a wavefront that is alone
// on its SIMD.  Here a workgroup of four wavefronts eliminates the interior frames e_1 .. e_q of a group in ceil(log2(q + 1)) rounds:
// e_1, e_3, e_5, e_7 at once, then e_2, e_6, then e_4 -- a frame's "separator" and "next" (chain_eliminate's X_s / X_n) are simply its left and
// right neighbour at that moment, i -+ 2^(round - 1), and the fill-in between the two neighbours is what the role-1 and role-3 lanes produce
// anyway.  Wavefront w holds e_{2w+1} and e_{2w+2}; after a round every lane leaves out[0..8] for the left and out[9..17] for the right
// neighbour in LDS (one image of 9 x 64 per source and side), ONE workgroup barrier, and the wavefront that holds a neighbour adds the left
// source's image, then the right one's (fixed order: bit-stable).  Border and A columns accumulate; the coupling columns are the fill-in of the
// round before the frame's own.  The wavefront of the last round (e_{2^(K-1)}: both of its neighbours are separators) finishes a and r as
// k_chain_fwd2's middle frame does: a absorbs the left-edge frames' updates in round order, r's update goes to the side image rw, the fill-in
// between a and r becomes a's B block.  Images: [Y | z | X_s (left neighbour) | L | X_n (right neighbour)]; the back-substitution follows the
// same order (chain_back_oe).  top: the chain's top level -- t <= 7 frames, no separators.
constexpr int kOeSlot = 9 * 64;                                  // one hand-over image: nine values per lane
constexpr int kOeWaveLds = 9 * kXsLd + 81 + 81 + 2;               // XS, An, Ls of one wavefront (344 doubles: 16-byte aligned)
constexpr int kOeLds = kOeWaves * kOeWaveLds + 8 * kOeSlot;       // doubles of LDS of a group's workgroup
// The image frame i leaves for its left (side 0) / right (side 1) neighbour.  The frames of round 1 own two images each; a frame of round 2
// writes into the two images it read itself after round 1 (its own program order keeps that safe); the last round's frame writes none.
// The kernels index a wavefront's frames, a round's sources and a round's frames in closed form (wave-uniform scalars, compile-time unrolling);
// every one of those forms is the schedule's, checked here against oe_full for the whole group: vc_chain_order.hpp stays the one definition.
constexpr bool oe_closed_forms_match() {
  for (int i = 1; i <= kOeMaxQ; ++i) {
    const OeFrame f = oe_full(i);
    const int h = 1 << (f.step - 1);
    if (f.wave != (i - 1) / 2) return false;                                            // wavefront w holds e_{2w+1}, e_{2w+2}
    if (i % h != 0 || ((i / h) & 1) != 1) return false;                                 // round k: the frames h (2u + 1), h = 2^(k-1)
    if (oe_slot(f.left) != i - h || oe_slot(f.right) != i + h) return false;            // neighbours i -+ h; slots 0 / kOeMaxQ + 1: the separators
    // the sources of frame i after round j < step: the frames of round j whose neighbour it is -- i -+ 2^(j-1)
    for (int j = 1; j < f.step; ++j) {
      const int hs = 1 << (j - 1);
      if (oe_full(i - hs).step != j || oe_slot(oe_full(i - hs).right) != i) return false;
      if (i + hs <= kOeMaxQ && (oe_full(i + hs).step != j || oe_slot(oe_full(i + hs).left) != i)) return false;
    }
  }
  for (int q = 1; q <= kOeMaxQ; ++q) {
    const OeFrame f = oe_frame(q, true, true, oe_last(q));
    if (f.step != oe_steps(q) || f.left != kOeLeftSep || f.right != kOeRightSep) return false;      // the last round's frame sees both separators
    for (int k = 1; k <= oe_steps(q); ++k) if (oe_frame(q, true, true, oe_left_edge(k)).left != kOeLeftSep || oe_frame(q, true, true, oe_left_edge(k)).step != k) return false;
  }
  for (int k = 1; k <= kOeMaxSteps; ++k) if (oe_full(oe_right_edge(k)).right != kOeRightSep || oe_full(oe_right_edge(k)).step != k) return false;
  return kOeWaves * 2 >= kOeMaxQ + 1 && kOeMaxQ == kChainM - 1;
}
static_assert(oe_closed_forms_match(), "the kernels' index arithmetic no longer matches vc_chain_order.hpp");
__device__ __forceinline__ int oe_image(int i, int side) {
  const int h = oe_low_bit(i);
  return h == 1 ? i - 1 + side : (side == 0 ? i - h / 2 : i + h / 2 - 1);
}
// The barrier between two rounds waits for LDS only: the wavefront's LDS stores have been performed (lgkmcnt(0); LDS operations of a wavefront
// execute in order), its global loads and stores stay in flight -- __syncthreads() carries a workgroup-scope fence that waits for the stores of
// the solved image as well (vc_kutil.hpp: wave_lds_sync_local; the idiom of k_chain_l0's and k_chain_back_path's ready words).  Nothing the
// wavefronts of a group hand each other goes through global memory: what one stores there is read by later launches, and what it loads (its
// frames' columns, the left frame's B block) has arrived before its first elimination, a barrier ahead of whoever overwrites it.
// Measured against __syncthreads() on one box: the levels the same, the top level's launch 12.3 against 13.0 us.
__device__ __forceinline__ void oe_round_barrier() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_s_waitcnt(0xc07f);          // lgkmcnt(0)
  __builtin_amdgcn_s_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}
__device__ __forceinline__ void chain_oe_group(const DevView& v, int s, int lvl, int top, int group, double* lds) {
  const int wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), lane = threadIdx.x & 63;
  const int N = v.n_frames, D = v.D, ldw = v.ldw, ldx = v.ldx, nW = D + 1, ncol = nW + 27;
  const long gs = (long)kChainM * s;
  const int a = top ? -1 : (int)((long)group * gs), first = top ? 0 : a + s;
  const int done = v.ctrl->done;
  if (lvl == 1 && blockIdx.x == 0 && threadIdx.x == 0) signal_started(v, 7);      // the bottom level is complete: this launch runs (the weight update waits for it)
  const bool pend = lvl > 0;
  const double* rp = v.rX[(lvl + 1) & 1];
  double* rw = v.rX[lvl & 1];
  const size_t isz = (size_t)9 * ldx;
  const int c = lane, e0 = c - nW;
  const int role = c < nW ? 0 : (e0 < 9 ? 1 : e0 < 18 ? 2 : e0 < 27 ? 3 : 4);     // 0 border (W | g), 1 C, 2 A, 3 B, 4 none
  const int pc = c < nW ? c : (c < ncol ? ldw + e0 : 0);
  const int sub = e0 < 9 ? e0 : e0 < 18 ? e0 - 9 : e0 - 18;
  if (first >= N) {            // a separator without interior frames: only its pending right contribution is folded in (uniform over the workgroup)
    if (!done && wv == 0 && !top && a < N) {
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
  const int q = top ? (N - 1) / s + 1 : min(kOeMaxQ, (N - 1 - first) / s + 1);      // interior frames e_1 .. e_q
  const int r = first + q * s;
  const bool has_l = !top, has_r = !top && q == kOeMaxQ && r < N;
  const int K = oe_steps(q), ilast = oe_last(q), wfin = (ilast - 1) / 2;
  const int ia = 2 * wv + 1, ib = 2 * wv + 2;                 // this wavefront's frames: round 1, and a later round
  const bool have_a = ia <= q, have_b = ib <= q;
  const int sb = oe_frame(q, has_l, has_r, ib).step;
  double* XS = lds + wv * kOeWaveLds; double* An = XS + 9 * kXsLd; double* Ls = An + 81;
  double* IMG = lds + kOeWaves * kOeWaveLds;
  // frame i of the group is base + i s; its pending image (the level below left it for a right separator) is number pq + i
  const int base = top ? -s : a, pq = top ? -1 : group * kChainM;
  const unsigned ldxb = 8u * (unsigned)ldx, iszb = 9u * ldxb;
  // (k_chain_fwd2's load pattern: one byte offset per lane -- first entry c0b, step stb -- from wave-uniform bases.  A frame of round 1 reads
  //  its own border, A and B columns and, as its coupling to the left, the row of the left frame's B block; a frame of a later round only
  //  border and A: its couplings arrive as fill-in)
  auto load_cols = [&](int i, bool round1, double* x) {
    const int e = base + i * s;
    const bool has_left = i > 1 || has_l;
    const bool tr = round1 && role == 1;                      // the left frame's B block, transposed
    const unsigned c0b = tr ? 8u * (unsigned)(sub * ldx + ldw + 18) : 8u * (unsigned)pc, stb = tr ? 8u : ldxb;
    const unsigned fb = (unsigned)((tr && has_left) ? e - s : e) * iszb, pb = (unsigned)(pq + i) * iszb;
    const bool live0 = role == 0 || role == 2 || (round1 && (role == 3 || (role == 1 && has_left)));
    const bool live1 = pend && e > 0 && (role == 0 || role == 2);
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
  double xa[9], xb[9], sep0[9];
#pragma unroll
  for (int k = 0; k < 9; ++k) { xa[k] = 0.0; xb[k] = 0.0; sep0[k] = 0.0; }
  // all of the wavefront's columns are requested now; so is what the left separator will absorb into (nobody else writes it during this level)
  if (have_a) load_cols(ia, true, xa);
  if (have_b) load_cols(ib, false, xb);
  // (every wavefront, branch-free like load_cols: behind a condition the compiler turned these into nine dependent round trips, each with a
  //  wait for everything in flight, at the head of the wavefront the last round depends on)
  {
    const bool pa = pend && a > 0, mine = has_l && wv == wfin && (role == 0 || role == 1);
    const int pcd = role == 1 ? ldw + 9 + sub : pc;
    const unsigned c0b = 8u * (unsigned)pcd;
    const unsigned ab = (unsigned)(has_l ? a : 0) * iszb, pab = (unsigned)(has_l ? a / s : 0) * iszb;
    double y0[9], y1[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) y0[k] = ld_boff(v.cW, ab + c0b + k * ldxb);
    if (pend) {
#pragma unroll
      for (int k = 0; k < 9; ++k) y1[k] = ld_boff(rp, pab + c0b + k * ldxb);
    } else {
#pragma unroll
      for (int k = 0; k < 9; ++k) y1[k] = 0.0;
    }
#pragma unroll
    for (int k = 0; k < 9; ++k) sep0[k] = mine ? y0[k] + (pa ? y1[k] : 0.0) : 0.0;
  }
  if (done) return;                      // (uniform over the workgroup: ahead of every barrier)
  const ElimLds elds = {XS, An, Ls};
  double out[18];
#pragma unroll
  for (int k = 0; k < 18; ++k) out[k] = 0.0;
  // EVERY wavefront runs every round and meets every barrier, with or without a frame of its own
  for (int st = 1; st <= K; ++st) {
    if (st > 1) {
      oe_round_barrier();                // the images of round st - 1 are complete
      if (have_b && sb >= st) {
        // e_ib receives from the two frames of round st - 1 beside it: left source (its right-going image), then right source (its left-going one)
        const int hs = 1 << (st - 2), il = ib - hs, ir = ib + hs;
        const bool has_rs = ir <= q, fin = sb == st;
        const double* L = IMG + oe_image(il, 1) * kOeSlot + c;
        const double* R = IMG + oe_image(has_rs ? ir : il, 0) * kOeSlot + (role == 2 ? c - 9 : c);      // (A's columns: the right source's C lanes carry their update)
        double fl[9], fr[9];           // (all eighteen reads first, then selects: no branch per role, one LDS round trip)
#pragma unroll
        for (int k = 0; k < 9; ++k) { fl[k] = L[k * 64]; fr[k] = R[k * 64]; }
#pragma unroll
        for (int k = 0; k < 9; ++k) {
          const double l = fl[k], r = has_rs ? fr[k] : 0.0;
          const double acc = (xb[k] - l) - r;                 // border and A: left source, then right source
          const double cpl = role == 1 ? -l : -r;             // coupling to the left / right neighbour: that side's fill-in of the round before
          xb[k] = (role == 0 || role == 2) ? acc : ((fin && (role == 1 || role == 3)) ? cpl : 0.0);
        }
      }
    }
    const int i = st == 1 ? (have_a ? ia : 0) : ((have_b && sb == st) ? ib : 0);      // wave-uniform; 0: nothing to eliminate this round
    if (i > 0) {
      double x[9];
#pragma unroll
      for (int k = 0; k < 9; ++k) x[k] = st == 1 ? xa[k] : xb[k];
      if (role == 2) {
#pragma unroll
        for (int k = 0; k < 9; ++k) An[k * 9 + sub] = x[k];
      }
      chain_eliminate<false>(v, v.cW + (size_t)(base + i * s) * isz, ldx, role, pc, sub, c == 0, elds, x, out);
      if (i != ilast) {
        double* L = IMG + oe_image(i, 0) * kOeSlot + c;
        double* R = IMG + oe_image(i, 1) * kOeSlot + c;
#pragma unroll
        for (int k = 0; k < 9; ++k) { L[k * 64] = out[k]; R[k * 64] = out[9 + k]; }
      }
    }
  }
  // ---- the last round's wavefront: out is e_ilast's; the separators' updates in round order
  if (wv != wfin || !has_l) return;
  double dl_[9], dr_[9];
#pragma unroll
  for (int k = 0; k < 9; ++k) { dl_[k] = 0.0; dr_[k] = 0.0; }
  for (int st = 1; st < K; ++st) {
    const double* L = IMG + oe_image(oe_left_edge(st), 0) * kOeSlot + c;
    const double* R = IMG + oe_image(oe_right_edge(st), 1) * kOeSlot + c;
#pragma unroll
    for (int k = 0; k < 9; ++k) { dl_[k] += L[k * 64]; if (has_r) dr_[k] += R[k * 64]; }
  }
  if (has_r && role < 4) {               // the right separator's side image
    double* ri = rw + (size_t)(r / gs) * isz + pc;
    const bool keep = role == 0 || role == 2;
#pragma unroll
    for (int k = 0; k < 9; ++k) ri[k * ldx] = keep ? -(dr_[k] + out[9 + k]) : 0.0;
  }
  if (role == 3) {                       // the separator's coupling to the right separator at the next level (none where the chain ends)
    double* img = v.cW + (size_t)a * isz + pc;
#pragma unroll
    for (int k = 0; k < 9; ++k) img[k * ldx] = has_r ? -out[k] : 0.0;
  }
  if (role == 0 || role == 1) {          // the left separator absorbs its group (the C lanes carry the update of A's columns)
    const int pcd = role == 1 ? ldw + 9 + sub : pc;
    double* img = v.cW + (size_t)a * isz + pcd;
#pragma unroll
    for (int k = 0; k < 9; ++k) img[k * ldx] = sep0[k] - (dl_[k] + out[k]);
  }
}

}  // namespace vc
