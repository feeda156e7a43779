#pragma once
// vc_chain_plan.hpp -- the level schedule of the partitioned chain elimination (chain_levels, vc_imu_kernels.hip; the levels' kernels in vci_chain_*.hpp) and the forms of the visual-inertial
// pass that follow from it, computed once per upload (vc_upload.cpp) from the problem's shape and the switches of DESIGN §9.  Every
// launcher, the pass (vc_pass.cpp), the buffer sizes and vc_pass_paths read this one plan.  Plain C++: the host test harness builds it.
#include <algorithm>

namespace vc {

constexpr int kChainM = 8;               // group size: 7 eliminations per wavefront and level
constexpr int kChainMaxLevels = 16;      // levels below the top one (a level multiplies the stride by kChainM)
constexpr int kChainEarlyTopD = 31;      // = kEarlyTopD (vc_device.h): k_reduced adds the top level's frames itself up to this width

// the tested switches that select forms of the pass (VICALIB_AMD_FOLD_L0, _BACK_PATH, _HADD_EARLY, _DEFER_TAIL, _CHAIN_ODD_EVEN; =0 turns one off)
struct ChainSwitches { bool fold_l0 = true, back_path = true, hadd_early = true, defer_tail = true, odd_even = true; };

struct ChainPlan {
  // strides 1, m, m^2, ... while more than m - 1 frames are active, then the top level (one wavefront eliminates the rest, stride top_stride)
  int n_levels = 0;
  int stride[kChainMaxLevels] = {}, m[kChainMaxLevels] = {}, groups[kChainMaxLevels] = {};
  // two[l]: level l is eliminated from both ends of its groups (k_chain_fwd2).  Narrow borders only (two columns per lane's worth, D <= 100):
  // two wavefronts per sweep, a whole CU per group -- on levels whose groups the chip holds at once (256; one-column borders: every level).
  // A function of the frame count and the level only: forward, backward and every hand-over mode agree on it.  (Measured 26.3 -> 21.7 us
  // per level at cfg3; the bottom level too, since the weight update on the other stream starts behind it -- vc_pass.cpp)
  int two[kChainMaxLevels] = {};
  // oe[l]: level l's groups are eliminated by odd-even reduction inside a workgroup of four wavefronts (k_chain_oe, vc_chain_order.hpp):
  // 3 dependent eliminations per level instead of the two sweeps' 4.  One-column borders, single-process passes, levels above the bottom one (whose builders occupy
  // the other two wavefronts); two[l] keeps its value -- it says what the level runs with the switch off.  oe_top: the top level likewise
  // (ceil(log2(t + 1)) eliminations for its t frames instead of t).
  int oe[kChainMaxLevels] = {};
  int oe_top = 0;
  int top_stride = 1;
  int forward_launches = 0;              // launches of the forward elimination (levels + the top level); 0: no frames
  int bottom_groups = 1;                 // groups of the bottom level (DevView::n_chain_groups)
  // forms of the pass (DevView fields of the same names; all 0 without the IMU)
  int fold_l0 = 0;                       // k_chain_init's work rides in the bottom level's launch (k_chain_l0)
  int gram_top_stride = 0;               // early Gram: the Gram sums ride in the top level's launch (0: k_chain_gram of its own)
  int back_path = 0;                     // the whole back-substitution in one launch (k_chain_back_path)
  int top_gram_launch = 0;               // early Gram: the top level's own frames need a Gram launch of their own (k_chain_gram(top))
  int hadd_early = 0;                    // the shared blocks of the reduced system as side jobs of the upper levels' launches
  int tail_deferred = 0;                 // the reduced solve's tail rides in the back-substitution's launch
};

// N frames, D shared columns, n_cams cameras; sharded: the pass has all-reduces (frame sharding with the IMU pins frames as well)
inline ChainPlan plan_chain(int N, int D, int n_cams, bool imu_on, bool sharded, const ChainSwitches& sw) {
  ChainPlan p;
  if (N < 1) return p;
  long st = 1;
  while ((N - 1) / st + 1 > kChainM - 1) {
    const int l = p.n_levels++;
    p.stride[l] = (int)st; p.m[l] = kChainM; p.groups[l] = (int)((N - 1) / (st * kChainM) + 1);
    st *= kChainM;
  }
  p.top_stride = (int)st;
  p.forward_launches = p.n_levels + 1;
  if (p.n_levels > 0) p.bottom_groups = p.groups[0];
  const int cpl = (D + 1 + 27 + 63) / 64;      // 64-column images of a frame's row (border + 27 chain columns) per lane
  for (int l = 0; l < p.n_levels; ++l) p.two[l] = (cpl <= 1 || (cpl <= 2 && p.groups[l] <= 256)) ? 1 : 0;
  // (never a sharded pass: those keep the two sweeps and the one-wavefront top level)
  for (int l = 1; l < p.n_levels; ++l) p.oe[l] = (sw.odd_even && !sharded && p.two[l] && cpl <= 1) ? 1 : 0;
  p.oe_top = (sw.odd_even && !sharded && cpl <= 1) ? 1 : 0;
  if (!imu_on) return p;
  // k_chain_l0 serves narrow borders, at most two cameras, at least one level below the top one; never a sharded pass.  A function of the
  // problem only, never of the hand-over mode; its chunk of the partial sums is the group of 8 frames
  p.fold_l0 = (sw.fold_l0 && !sharded && D + 1 + 27 <= 64 && n_cams <= 2 && p.n_levels >= 1) ? 1 : 0;
  // early Gram where it pays: the top level's one group must outlast the Gram sums beside it -- at 6250 frames x 8 cameras, D = 115, the top
  // level is two frames and the sums take 50 us: 0.906 -> 0.938 ms per pass with them in its launch; at 2500 frames, D = 67: -4.5 us
  p.gram_top_stride = (N <= 4096 && D + 1 + 27 <= 128) ? p.top_stride : 0;
  // every bottom group of k_chain_back_path recomputes the levels above it: (levels + 1) x the level-by-level form's work -- free while the
  // bottom groups fit the chip in one round, 120 us against 71 at 6250 frames x D = 115 (profiles/r06_per_rank_passes.txt): up to 4096 frames
  p.back_path = (sw.back_path && N <= 4096) ? 1 : 0;
  p.top_gram_launch = (p.gram_top_stride > 0 && !(D <= kChainEarlyTopD && !sharded)) ? 1 : 0;
  // the side jobs need a two-sided level 1 (the sums behind S and g_red) and the early-Gram top level (the record itself)
  p.hadd_early = (sw.hadd_early && p.gram_top_stride > 0 && p.n_levels >= 2 && p.two[1]) ? 1 : 0;
  // the tail needs k_chain_back_path's workgroups of at least 256 threads (levels + 1 wavefronts)
  p.tail_deferred = (sw.defer_tail && p.back_path && p.n_levels >= 3 && p.n_levels <= 5) ? 1 : 0;
  return p;
}

}  // namespace vc
