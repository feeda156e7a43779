#pragma once
// vc_chain_order.hpp -- the order in which the interior frames of ONE group of the partitioned chain elimination are eliminated by odd-even
// reduction inside a workgroup (vci_chain_oe.hpp: chain_oe_group under k_chain_oe and the top level; vc_imu_kernels.hip: the three back-substitution kernels), and who a frame's
// neighbours are when its turn comes.  Plain C++ for host and device: the host test harness builds it (tests/host_harness).
//
// A group is [a | e_1 .. e_q | r]: q = 1 .. 7 interior frames, a left separator a and a right separator r that may each be absent (the
// chain's top level has neither).  Interior index i goes at step k where 2^(k-1) is the largest power of two dividing i; its neighbours at
// that moment are i - 2^(k-1) and i + 2^(k-1) -- an index that falls off the group is the separator of that side, or nobody if that side has
// none.  Frames of one step are never neighbours of each other, so a step is one round of independent eliminations: ceil(log2(q + 1)) rounds
// instead of q (one sweep) or (q + 1) / 2 + 1 (two sweeps).  The last round is always frame 2^(K-1) alone.
// Wavefront w of the group's workgroup eliminates e_{2w+1} and then e_{2w+2}: consecutive indices never share a step, and a wavefront holds
// at most the columns of two frames.

#if defined(__HIPCC__) || defined(__CUDACC__)
#define VC_ORDER_HD __host__ __device__
#else
#define VC_ORDER_HD
#endif

namespace vc {

constexpr int kOeMaxQ = 7;            // interior frames of a group at most (kChainM - 1)
constexpr int kOeMaxSteps = 3;        // ceil(log2(kOeMaxQ + 1))
constexpr int kOeWaves = 4;           // wavefronts of a group's workgroup
// a neighbour: an interior index 1 .. q, or one of
constexpr int kOeLeftSep = 0, kOeRightSep = -1, kOeNobody = -2;

struct OeFrame { int step, left, right, wave; };      // step 1 .. ; left / right: neighbours at elimination time; wave 0 .. kOeWaves - 1

VC_ORDER_HD constexpr int oe_low_bit(int i) { return i & -i; }
VC_ORDER_HD constexpr int oe_steps(int q) { int k = 0; while ((1 << k) < q + 1) ++k; return k; }
VC_ORDER_HD constexpr OeFrame oe_frame(int q, bool has_left, bool has_right, int i) {
  const int h = oe_low_bit(i);
  int k = 1;
  while ((1 << (k - 1)) < h) ++k;
  const int l = i - h, r = i + h;
  return OeFrame{k, l >= 1 ? l : (has_left ? kOeLeftSep : kOeNobody), r <= q ? r : (has_right ? kOeRightSep : kOeNobody), (i - 1) / 2};
}
// The kernels unroll the FULL group's order (q = kOeMaxQ, both separators) with compile-time indices and keep one slot per position
// 0 (a), 1 .. 7, 8 (r): a shorter group or a missing separator is the same order with those slots absent (zero) -- oe_frame's clipping.
VC_ORDER_HD constexpr int oe_slot(int nb) { return nb == kOeRightSep ? kOeMaxQ + 1 : nb; }      // (kOeNobody has no slot)
VC_ORDER_HD constexpr OeFrame oe_full(int i) { return oe_frame(kOeMaxQ, true, true, i); }
// the frame of the last round (the one that touches both separators), and the frame of round k whose left / right neighbour is the separator
VC_ORDER_HD constexpr int oe_last(int q) { return 1 << (oe_steps(q) - 1); }
VC_ORDER_HD constexpr int oe_left_edge(int k) { return 1 << (k - 1); }
VC_ORDER_HD constexpr int oe_right_edge(int k) { return kOeMaxQ + 1 - (1 << (k - 1)); }      // (a full group's: only that one has a right separator in the chain)

}  // namespace vc
