// vc_imu_kernels.hip -- inertial stages of the LM engine (gfx950, wave64).
//
// With IMU blocks in the problem (SetupProblem, vicalibrator.h:607-637, :651-655) consecutive frames are
// coupled, so the per-frame elimination of the vision-only path becomes the factorisation of a
// block-tridiagonal chain (9 x 9 blocks: pose 6 + velocity 3) bordered by the shared parameters.
//
// The IMU stages, the chain assembly and the levels of the elimination stand in stage fragments (vci_*.hpp, each with its own description),
// included below in the order of a pass; they define __global__ symbols and belong to this translation unit alone.  The folded bottom level,
// the back-substitution and the Gram sums follow in this file, then the launchers.
//  k_imu_jac       vci_imu_jac.hpp      IMU residual, Cauchy weight and the block's weighted J^T J / J^T r
//  k_imu_block     vci_imu_block.hpp    the pose-independent part of the preintegration (block deltas)
//  k_imu_weights   vci_imu_weights.hpp  UpdateImuWeights, interval-parallel
//  k_chain_init    vci_chain_init.hpp   chain assembly: the frames' images, damping, chunk sums
//  k_chain_fwd     vci_chain_fwd.hpp    one level of the partitioned elimination, one sweep per group
//  k_chain_fwd2    vci_chain_fwd2.hpp   ... from both ends of the group at once (chain_eliminate)
//  k_chain_oe      ... by odd-even reduction inside a workgroup of four wavefronts (chain_oe_group: vci_chain_oe.hpp; the kernel: behind
//                  k_chain_top_gram below)
//  k_chain_gram    sum over all frames of [Y | z]^T [Y | z] on the matrix pipe (v_mfma_f64_16x16x4_f64)
//  k_chain_l0      (round 5) k_chain_init's work and the bottom level of the elimination in one launch: the frames' images stay in LDS
//                  (narrow borders, at most two cameras, single process)
//  k_chain_top_gram  the top level of the elimination and, beside it in the same launch, k_chain_gram's sums of the frames below it
//  k_chain_back    back-substitution, one level per launch; the bottom level also writes the trial poses / velocities
//  k_chain_back_levels  ... all levels below the top in one launch (ready words between the workgroups)
//  k_chain_back_path    (round 5) the whole back-substitution in one launch without hand-overs: a workgroup per bottom-level group
//                  recomputes the levels above it (narrow borders, single process)
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdlib>
#include "vc_math.hpp"
#include "vc_imu.hpp"
#include "vc_imu_weights.hpp"
#include "vc_device.h"
#include "vc_chain_order.hpp"
#include "vc_kutil.hpp"
#include "vc_reduced_tail.hpp"      // (k_chain_back_path, below; vc_shared_blocks.hpp comes with vci_chain_fwd2.hpp, its first user)

// (the order is part of the build: the code object lists the kernels in definition order, and a device function that is not
//  __forceinline__ must stay ahead of its callers)
#include "vci_imu_jac.hpp"          // kImuJacLds, SegInv / d_seg_inv, k_imu_jac
#include "vci_lanes.hpp"            // DPP row operations, delta / map scans over lanes, imu_range_lanes, imu_view
#include "vci_imu_block.hpp"        // delta_t_pack / unpack / scan_level, k_imu_block
#include "vci_imu_weights.hpp"      // k_imu_weights
#include "vci_chain_init.hpp"       // InitLoads, k_chain_init
#include "vci_chain_fwd.hpp"        // kXsLd, chain_fwd_group, k_chain_fwd
#include "vci_chain_fwd2.hpp"       // ld_boff, chain_eliminate, k_chain_fwd2
#include "vci_chain_oe.hpp"         // oe_closed_forms_match, oe_image, oe_round_barrier, chain_oe_group

namespace vc {

// ---- bottom level with the chain assembly folded in (round 5; verdict r3 / r4 item 1a) ---------------------------------------------------
// One workgroup of FOUR wavefronts per group of 8 frames [a | e_1 .. e_7 | (r)]: wavefronts 0 / 1 are k_chain_fwd2<1>'s two sweeps,
// wavefronts 2 / 3 are BUILDERS that do k_chain_init's work for the group's frames in the order the sweeps need them (builder 2: the left
// sweep's frames, then the middle; builder 3: the right sweep's frames, then the separator a) and hand every frame over through LDS: the
// border [W | g] and the block A of an unsolved frame never touch HBM (k_chain_init wrote the image, the bottom level read it back, a kernel
// boundary between them).  The 9 x 9 couplings B -- all an image needs besides -- are read by the sweeps straight from the IMU block records.
// A builder requests its next frame's records before it forms the current frame's columns, so the sweeps wait ~one frame's build at their
// start and the builders stay ahead from there.  The frame's solved image, the damping state and the chunk sums (chunk = group) go to HBM as
// before.  Narrow borders (one image column per lane), at most two cameras, single process (no pinned frames), groups of 8, two-sided.
constexpr int kL0Ld = 48;      // row stride of a frame's LDS image: border (D + 1 <= 37 columns), then the 9 columns of A
template <int CMAX>
__global__ __launch_bounds__(256) void k_chain_l0(DevView v) {
  constexpr int W = 64;
  __shared__ __attribute__((aligned(16))) double XS2[2][9 * kXsLd];
  __shared__ double An2[2][81], Ls2[2][81];
  __shared__ double MID[9 * W], SEPR[9 * W];
  __shared__ double IMG[8][9 * kL0Ld];
  __shared__ int READY[12];              // [slot]: the frame's image is in IMG; [8 + w], w = 0, 1, 3: wavefront w's chunk sums are in SUMW
  __shared__ double BW[4][CMAX * kGStride + kInitPad];
  __shared__ double SUMW[4][CMAX * kGStride + kGStride + 16];
  __shared__ CamDesc s_cd2[4][kMaxCams];      // every wavefront keeps its own small tables: no workgroup barrier between the start and the
  __shared__ double s_R2[4][kMaxCams * 9];    // first frames (the one barrier ahead of everything only publishes READY = 0)
  const int tid = threadIdx.x, wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), lane = threadIdx.x & 63, group = blockIdx.x;
#ifdef VC_L0_STAMPS
  const long long l0t0_ = (long long)__builtin_amdgcn_s_memrealtime();
  int l0n_ = 1;
#define L0STAMP() do { if (blockIdx.x == gridDim.x / 2 && lane == 0 && l0n_ < 16) { v.dbg[(wv == 0 ? 0 : 16) + l0n_] = (long long)__builtin_amdgcn_s_memrealtime(); ++l0n_; } } while (0)
#define L0B(i) do { if (blockIdx.x == gridDim.x / 2 && lane == 0 && wv == 2 && it == 1) v.dbg[24 + (i)] = (long long)__builtin_amdgcn_s_memrealtime(); } while (0)
#else
#define L0STAMP() do { } while (0)
#define L0B(i) do { } while (0)
#endif
  const int N = v.n_frames, D = v.D, C = v.n_cams, ldw = v.ldw, ldx = v.ldx, nW = D + 1, ncol = nW + 27;
  const Ctrl* ct = v.ctrl;
  const int a = group * 8, first = a + 1;
  const int q = first < N ? min(7, N - 1 - first + 1) : 0;     // interior frames e_1 .. e_q
  const int r = first + q;
  const bool has_r = q == 7 && r < N;
  const int nl = q > 0 ? (q - 1) / 2 : 0, mid = nl + 1, nr = q > 0 ? q - 1 - nl : 0;
  const size_t isz = (size_t)9 * ldx;
  // Hand-over through LDS only.  A workgroup-scope fence would also wait for the wavefront's outstanding GLOBAL loads and stores -- the
  // builder's requests for its next frames, the sweep's stores of the image it has just solved (1.7 us per frame, measured): here the
  // producer waits for its own LDS stores (lgkmcnt(0), nothing else) before it raises the word, the consumer's LDS reads follow its poll
  // in the wavefront's LDS queue, and wavefront-scope fences keep the compiler from moving LDS accesses across either.
  auto wait_ready = [&](int slot) {
    while (__hip_atomic_load(&READY[slot], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) == 0) __builtin_amdgcn_s_sleep(1);
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    __builtin_amdgcn_wave_barrier();
  };
  auto set_ready = [&](int slot) {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_s_waitcnt(0xc07f);          // lgkmcnt(0): this wavefront's LDS stores have been performed
    __builtin_amdgcn_wave_barrier();
    if (lane == 0) __hip_atomic_store(&READY[slot], 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
  };
  if (tid < 12) READY[tid] = 0;
  __syncthreads();
  // ---- the builders' first requests go out before anything else: the tile list of their first frame ahead of the control record, the
  // frame's records as soon as that record says which linearisation buffer is current -- under the tables and the barrier below
  // Who builds what (round 5, second cut): the SWEEPS build their own first frame -- they would only wait for it -- while the builders
  // already work on the second ones: wavefront 0 the first frame of the left sweep (the middle if there is none), wavefront 1 the first of
  // the right sweep, builder 2 the rest of the left sweep's frames and then the middle, builder 3 the rest of the right sweep's and then
  // the separator a.  (With the builders alone the sweeps ran at the builders' ~4 us per frame instead of their own 2.8.)
  const int b = wv;                                                // (index of this wavefront's scratch and tables)
  const int nmine = q == 0 ? (wv == 3 ? 1 : 0)
                  : wv == 0 ? 1 : wv == 1 ? (nr > 0 ? 1 : 0) : wv == 2 ? (nl > 0 ? nl : 0) : (nr > 0 ? nr - 1 : 0) + 1;
  auto slot_of = [&](int i) {
    return q == 0 ? 0 : wv == 0 ? (nl > 0 ? 1 : mid) : wv == 1 ? q : wv == 2 ? (i < nl - 1 ? 2 + i : mid) : (i < nr - 1 ? q - 1 - i : 0);
  };
  int sp_col = -1;
#pragma unroll
  for (int a2 = 0; a2 < 15; ++a2) sp_col = (lane == a2) ? v.imu_param_col[a2] : sp_col;
  auto load_fct = [&](int f) { return (lane < C && f < N) ? v.frame_cam_tile[(size_t)f * C + lane] : -1; };
  int fctA = -1, fctB = -1;                                      // tile lists of the builder's first two frames
  if (nmine > 0) fctA = load_fct(a + slot_of(0));
  if (nmine > 1) fctB = load_fct(a + slot_of(1));
  if (ct->done) return;                                          // (uniform over the workgroup)
  const int cur = ct->cur;
  const double* segc = v.segb[cur];
  const int init_scale = ct->init_scale, reuse = ct->reuse_diag;
  const double radius = ct->radius;
  // per-lane offsets into a frame's two IMU records, once for all frames (the records' bases are wave-uniform: scalar base + 32-bit
  // lane offset per load, no 64-bit address arithmetic per lane and load -- issuing a frame's ~45 loads took 1.2 us of the builder's 4)
  const bool par = lane < 15 && sp_col >= 0;
  const int o_wc = par ? kSegWc + lane : 0, o_wp = par ? kSegWp + lane : 0, s_par = par ? 15 : 0;
  const int o_acc0 = kSegAcc + lane, o_acc1 = kSegAcc + (lane + 64 < 81 ? lane + 64 : 0), o_app0 = kSegApp + lane, o_app1 = kSegApp + (lane + 64 < 81 ? lane + 64 : 0);
  const int l9 = lane < 9 ? lane : 0;
  int o_ii[4];
#pragma unroll
  for (int qq = 0; qq < 4; ++qq) { const int e = lane + 64 * qq, a2 = e >> 4, b2 = e & 15; o_ii[qq] = a2 < 15 ? ((b2 < 15) ? kSegHii + a2 * 15 + b2 : kSegGi + a2) : 0; }
  auto issue = [&](int f_in, int fct_f, InitLoads<CMAX>& R) {
    const int f = __builtin_amdgcn_readfirstlane(f_in);
    const bool has_c = f >= 1, has_p = f + 1 < N;                               // wave-uniform
    // (an absent record: the base falls back to record 0 -- always there for N >= 2 -- and every value is dropped by its select)
    const double* rcs = segc + (size_t)(has_c ? f - 1 : 0) * kSegStride;
    const double* rps = segc + (size_t)(has_p ? f : 0) * kSegStride;
#pragma unroll
    for (int cc = 0; cc < CMAX; ++cc) {
      const int tc = __builtin_amdgcn_readfirstlane(__shfl(fct_f, cc, 64));
#pragma unroll
      for (int qq = 0; qq < 3; ++qq) R.gv[cc][qq] = 0.0;
      if (cc < C && tc >= 0) {
        const double* g = v.Gb[cur] + (size_t)tc * kGPack;
#pragma unroll
        for (int qq = 0; qq < 3; ++qq) { const int e = qq * 64 + lane; const double x = g[e < kGPack ? e : 0]; R.gv[cc][qq] = e < kGPack ? x : 0.0; }
      }
    }
    {
      const bool tile_cost = lane < C && fct_f >= 0, blk_cost = lane == 8 && has_c;
      const double* pcst = tile_cost ? v.tile_costb[cur] + fct_f : (blk_cost ? v.seg_costb[cur] + (f - 1) : v.cg);
      const double x = *pcst;
      R.cost_in = (tile_cost || blk_cost) ? x : 0.0;
    }
    double xa[9], xb[9], xc0, xc1, xp0, xp1, xi[4];
#pragma unroll
    for (int i = 0; i < 9; ++i) { xa[i] = rcs[o_wc + i * s_par]; xb[i] = rps[o_wp + i * s_par]; }
    xc0 = rcs[o_acc0]; xc1 = rcs[o_acc1]; xp0 = rps[o_app0]; xp1 = rps[o_app1];
    const double gc = rcs[kSegGc + l9], gp = rps[kSegGp + l9], s2 = v.cscale2[(size_t)f * 9 + l9], dgv = v.cdiag[(size_t)f * 9 + l9];
#pragma unroll
    for (int qq = 0; qq < 4; ++qq) xi[qq] = rcs[o_ii[qq]];
#pragma unroll
    for (int i = 0; i < 9; ++i) R.pre[i] = ((par && has_c) ? xa[i] : 0.0) + ((par && has_p) ? xb[i] : 0.0);
    const bool in1 = lane + 64 < 81, in9 = lane < 9;
    R.a_imu[0] = (has_c ? xc0 : 0.0) + (has_p ? xp0 : 0.0);
    R.a_imu[1] = ((in1 && has_c) ? xc1 : 0.0) + ((in1 && has_p) ? xp1 : 0.0);
    R.g_imu = ((in9 && has_c) ? gc : 0.0) + ((in9 && has_p) ? gp : 0.0);
    R.sc2_in = (in9 && !init_scale) ? s2 : 0.0;
    R.dg_in = (in9 && reuse) ? dgv : 0.0;
#pragma unroll
    for (int qq = 0; qq < 4; ++qq) R.isum_in[qq] = ((lane + 64 * qq) < 240 && has_c) ? xi[qq] : 0.0;
  };
  // two frames' records in flight (two register sets): a frame's loads are requested BEHIND the hand-over of the frame two before it --
  // issuing them (1.3 us of instructions) no longer sits between a frame's arrival and its hand-over
  InitLoads<CMAX> RA, RB;
  if (nmine > 0) issue(a + slot_of(0), fctA, RA);
  if (nmine > 1) issue(a + slot_of(1), fctB, RB);
  // the builder's own tables (camera descriptors, rotations R_ck) and what its lane's column is -- under its first frame's loads
  int col_ci = 0;
  if (nmine > 0) {                                                 // (wave-uniform)
    if (lane < kMaxCams) s_cd2[b][lane] = v.cd[lane];
    if (lane < C) { double Rm[9]; quat_to_R(v.cams[cur] + (size_t)lane * kCamStride, Rm); for (int k2 = 0; k2 < 9; ++k2) s_R2[b][lane * 9 + k2] = Rm[k2]; }
    if (lane < ncol) {
      const int col = lane, e = col - nW;
      int cam = 255, loc = 0, skip = (e >= 18 && e < 27) ? 1 : 0;
      if (col < D) {
        const int cc = v.col_cam[col];
        cam = cc >= 0 ? cc : 255; loc = v.col_local[col];
#pragma unroll
        for (int a2 = 0; a2 < 15; ++a2) skip |= (v.imu_param_col[a2] == col) ? 1 : 0;
      }
      col_ci = cam | (loc << 8) | (skip << 16);
    }
    wave_lds_sync_local();
  }
  // ============================================================ building (k_chain_init's work, frame by frame; all four wavefronts) ====
  double* Gw = BW[b];
  double* Hs = Gw + C * kGStride;
  double* As = Hs + 42;
  double* gs = As + 81;
  double* ls = gs + 9;
  int* tcam = reinterpret_cast<int*>(ls + 9);
  int* tinv = tcam + kMaxCams;
  double gsum[CMAX][3];
  double isum[4] = {0.0, 0.0, 0.0, 0.0};
  double csum = 0.0;
  int po[3], pm[3];
#pragma unroll
  for (int qq = 0; qq < 3; ++qq) {
    const int e = qq * 64 + lane;
    int rr = 0;
#pragma unroll
    for (int a2 = 1; a2 < 16; ++a2) rr += (e >= a2 * 16 - (a2 * (a2 - 1)) / 2) ? 1 : 0;
    const int cidx = rr + (e - (rr * 16 - (rr * (rr - 1)) / 2));
    po[qq] = e < kGPackGrad ? rr * 16 + cidx : (e < kGPack ? kGGrad + (e - kGPackGrad) : -1);
    pm[qq] = (e < kGPackGrad && cidx != rr) ? cidx * 16 + rr : -1;
  }
#pragma unroll
  for (int cc = 0; cc < CMAX; ++cc)
#pragma unroll
    for (int qq = 0; qq < 3; ++qq) gsum[cc][qq] = 0.0;
  // what this lane's image column is (one column per lane: D + 28 <= 64), once for all frames -- the column phase then runs without a
  // divergent branch: a camera's column is three weighted entries per row of its tile's Gram block (a rotation column: -R's column over
  // entries 3..5; a unit column: one entry with weight 1), A's and g's columns come from the frame's own block; everybody loads from valid
  // addresses and keeps what is his by selects.  (As `if (camera column) { if (rotation) .. else .. } if (g) .. if (A) ..` the phase took
  // 2.2 of the ~4 us a builder needs per frame: five serialised branch regions, each with its own LDS round trips.)
  int ckind = 0, ccam = 0, cjb = 0, cidx0 = 0, cidx1 = 0, cidx2 = 0, cic = 0;
  double cw0 = 0.0, cw1 = 0.0, cw2 = 0.0, cR[9];
#pragma unroll
  for (int i = 0; i < 9; ++i) cR[i] = 0.0;
  if (nmine > 0 && lane < ncol) {
    const int col = lane, ci = col_ci, e = col - nW;
    const int cc = ci & 255, j = (ci >> 8) & 255;
    cic = col < nW ? col : nW + (e >= 0 ? e % 9 : 0);
    cjb = (e >= 0) ? e % 9 : 0;
    if ((ci >> 16) || (e >= 0 && e < 9)) ckind = 0;             // IMU-record columns (written with the records' values), C, B
    else if (col == D) ckind = 2;
    else if (e >= 9 && e < 18) ckind = 3;
    else if (col < D && cc < kMaxCams) {
      ckind = 1; ccam = cc;
      const int flags = s_cd2[b][cc].flags, nrot = (flags & kCamRotFree) ? 3 : 0, ntr = (flags & kCamTransFree) ? 3 : 0;
      const double* Rm = s_R2[b] + cc * 9;
#pragma unroll
      for (int i = 0; i < 9; ++i) cR[i] = Rm[i];
      if (j < nrot) { cidx0 = 3; cidx1 = 4; cidx2 = 5; cw0 = -Rm[j]; cw1 = -Rm[3 + j]; cw2 = -Rm[6 + j]; }
      else { const int jj = (j < nrot + ntr) ? j - nrot : 6 + (j - nrot - ntr); cidx0 = jj; cidx1 = jj; cidx2 = jj; cw0 = 1.0; }
    } else if (col < nW) ckind = 4;                                // a border column nobody owns: zeros
  }
  auto build = [&](int it, InitLoads<CMAX>& R, int& fct) {
    const int slot = slot_of(it), f = a + slot;
    double* im = IMG[slot];
    const int fct2 = (it + 2 < nmine) ? load_fct(a + slot_of(it + 2)) : -1;      // the tile list of the frame that takes this register set next
    L0B(0);
    const unsigned long long present = __ballot(lane < C && fct >= 0);
    const int nt = __popcll(present);
    if (lane < kMaxCams) {
      const bool have = lane < C && fct >= 0;
      tinv[lane] = have ? __popcll(present & ((1ull << lane) - 1ull)) : -1;
    }
    wave_lds_sync_local();
    if (lane < C && fct >= 0) tcam[tinv[lane]] = lane;
    csum += R.cost_in;
#pragma unroll
    for (int qq = 0; qq < 4; ++qq) isum[qq] += R.isum_in[qq];
    int slot_c = 0;
#pragma unroll
    for (int cc = 0; cc < CMAX; ++cc) {
      const bool have = cc < C && ((present >> cc) & 1ull);
      if (have) {
#pragma unroll
        for (int qq = 0; qq < 3; ++qq) {
          if (po[qq] >= 0) Gw[slot_c * kGStride + po[qq]] = R.gv[cc][qq];
          if (pm[qq] >= 0) Gw[slot_c * kGStride + pm[qq]] = R.gv[cc][qq];
          gsum[cc][qq] += R.gv[cc][qq];
        }
        ++slot_c;
      }
    }
    if (sp_col >= 0) {          // the IMU-parameter columns of the border, straight from the records
#pragma unroll
      for (int i = 0; i < 9; ++i) im[i * kL0Ld + sp_col] = R.pre[i];
    }
    const double a_imu[2] = {R.a_imu[0], R.a_imu[1]};
    const double g_imu = R.g_imu, sc2_in = R.sc2_in, dg_in = R.dg_in;
    wave_lds_sync_local();
    L0B(1);
    L0B(2);
    if (lane < 42) {
      double hval = 0.0;
      for (int t = 0; t < nt; ++t) {
        const int cc = tcam[t];
        const double* Rm = s_R2[b] + cc * 9;
        const double* g = Gw + t * kGStride;
        if (lane < 36) {
          const int i = lane / 6, j = lane % 6, a2 = i / 3, ii = i % 3, b2 = j / 3, jj = j % 3;
          double sacc = 0.0;
#pragma unroll
          for (int pp = 0; pp < 3; ++pp)
#pragma unroll
            for (int qq = 0; qq < 3; ++qq) sacc += Rm[3 * pp + ii] * g[(3 * a2 + pp) * 16 + 3 * b2 + qq] * Rm[3 * qq + jj];
          hval += (a2 == b2) ? sacc : -sacc;
        } else {
          const int i = lane - 36, a2 = i / 3, ii = i % 3;
          const int nk = model_nk(s_cd2[b][cc].model);
          double sacc = 0.0;
#pragma unroll
          for (int pp = 0; pp < 3; ++pp) sacc += Rm[3 * pp + ii] * gram_grad(g, 3 * a2 + pp, nk);
          hval += (a2 == 0) ? -sacc : sacc;
        }
      }
      Hs[lane] = hval;
    }
    wave_lds_sync_local();
    L0B(3);
    double aval[2];
#pragma unroll
    for (int qq = 0; qq < 2; ++qq) {
      const int e = lane + 64 * qq, i = e / 9, j = e % 9;
      aval[qq] = a_imu[qq] + ((e < 81 && i < 6 && j < 6) ? Hs[i * 6 + j] : 0.0);
      if (e < 81) As[e] = aval[qq];
    }
    const double gval = g_imu + ((lane < 6) ? Hs[36 + lane] : 0.0);
    double hd = 0.0;
#pragma unroll
    for (int i = 0; i < 9; ++i) {
      const int e = i * 10;
      const double d = readlane_f64(aval[e >> 6], e & 63);
      if (lane == i) hd = d;
    }
    if (lane < 9) {
      double sc2 = sc2_in, dg = dg_in;
      if (init_scale) { sc2 = jacobi_scale2(hd); v.cscale2[(size_t)f * 9 + lane] = sc2; }
      if (!reuse) { dg = lm_clamped_diag(hd, sc2); v.cdiag[(size_t)f * 9 + lane] = dg; }
      const double lam = dg / (radius * sc2);
      v.clam[(size_t)f * 9 + lane] = lam;
      v.cg[(size_t)f * 9 + lane] = gval;
      gs[lane] = gval; ls[lane] = lam;
    }
    wave_lds_sync_local();
    L0B(4);
    // the image's border and A columns -> LDS (branch-free, see the lane constants above)
    {
      const int t = tinv[ccam];
      const double* g = Gw + (t >= 0 ? t : 0) * kGStride;
      double g0[6], g1[6], g2[6], av[9], gv9[9];
#pragma unroll
      for (int rr = 0; rr < 6; ++rr) { g0[rr] = g[rr * 16 + cidx0]; g1[rr] = g[rr * 16 + cidx1]; g2[rr] = g[rr * 16 + cidx2]; }
#pragma unroll
      for (int i = 0; i < 9; ++i) { av[i] = As[i * 9 + cjb]; gv9[i] = gs[i]; }
      const double lj = ls[cjb];
      double u[6];
#pragma unroll
      for (int rr = 0; rr < 6; ++rr) u[rr] = g0[rr] * cw0 + g1[rr] * cw1 + g2[rr] * cw2;
      double val[9];
#pragma unroll
      for (int i = 0; i < 3; ++i) {
        val[i] = -(cR[i] * u[0] + cR[3 + i] * u[1] + cR[6 + i] * u[2]);
        val[3 + i] = cR[i] * u[3] + cR[3 + i] * u[4] + cR[6 + i] * u[5];
        val[6 + i] = 0.0;
      }
      const bool cam_live = ckind == 1 && t >= 0;
#pragma unroll
      for (int i = 0; i < 9; ++i) {
        const double x = cam_live ? val[i] : (ckind == 2 ? gv9[i] : (ckind == 3 ? av[i] + ((i == cjb) ? lj : 0.0) : 0.0));
        if (ckind != 0) im[i * kL0Ld + cic] = x;
      }
    }
    L0B(5);
    set_ready(slot);
    L0B(6);
    if (wv == 2) L0STAMP();                 // builder 2: frame handed over
    fct = fct2;
    if (it + 2 < nmine) issue(a + slot_of(it + 2), fct, R);
  };
  for (int it = 0; it < nmine; it += 2) {
    build(it, RA, fctA);
    if (it + 1 < nmine) build(it + 1, RB, fctB);
  }
#ifdef VC_L0_STAMPS
  if (blockIdx.x == gridDim.x / 2 && lane == 0 && (wv == 0 || wv == 2)) v.dbg[wv == 0 ? 0 : 16] = l0t0_;
  if (wv == 0 || wv == 2) L0STAMP();      // 1: behind the first barrier
#endif
  if (wv < 2) {
    // ======================================================= the two sweeps (k_chain_fwd2<1> at s = 1, level 0) =======================
    // this sweep's own frame's contribution to the chunk sums: to LDS for builder 2, which needs it at the very end -- published where the
    // sweep has time (at the hand-over barrier), not between its frame's build and its first elimination
    auto publish_sums = [&]() {
      const int nsum_ = C * kGStride + kGStride;
#pragma unroll
      for (int cc = 0; cc < CMAX; ++cc)
        if (cc < C) {
#pragma unroll
          for (int qq = 0; qq < 3; ++qq) {
            if (po[qq] >= 0) SUMW[wv][cc * kGStride + po[qq]] = gsum[cc][qq];
            if (pm[qq] >= 0) SUMW[wv][cc * kGStride + pm[qq]] = gsum[cc][qq];
          }
        }
#pragma unroll
      for (int qq = 0; qq < 4; ++qq) SUMW[wv][C * kGStride + qq * 64 + lane] = isum[qq];
      if (lane < 9) SUMW[wv][nsum_ + lane] = csum;
      set_ready(8 + wv);
    };
    const int wave = wv;
    const int c = lane, e0 = c - nW;
    const int role = c < nW ? 0 : (e0 < 9 ? 1 : e0 < 18 ? 2 : e0 < 27 ? 3 : 4);     // 0 border (W | g), 1 C, 2 A, 3 B, 4 none
    const int pc = c < nW ? c : (c < ncol ? ldw + e0 : 0);
    const int sub = e0 < 9 ? e0 : e0 < 18 ? e0 - 9 : e0 - 18;
    const int icol = role == 0 ? c : nW + sub;                                       // the lane's column in an LDS image (roles 0, 2; role 1 lanes: A's column `sub`)
    if (q == 0) {              // a separator without interior frames: its image as the builders formed it, no coupling to the right
      if (wave == 0 && a < N) {
        wait_ready(0);
        double* img = v.cW + (size_t)a * isz;
        if (role == 0 || role == 2) {
#pragma unroll
          for (int k = 0; k < 9; ++k) img[k * ldx + pc] = IMG[0][k * kL0Ld + icol];
        } else if (role == 3) {
#pragma unroll
          for (int k = 0; k < 9; ++k) img[k * ldx + pc] = 0.0;
        }
      }
      return;
    }
    const int dir = wave == 0 ? 1 : -1, cnt = wave == 0 ? nl : nr, i0 = wave == 0 ? 1 : q;
    double* XS = XS2[wave]; double* An = An2[wave]; double* Ls = Ls2[wave];
    // the image columns of frame e as this sweep needs them: border and A from the builders' LDS image, the couplings from the IMU block
    // records (B of frame f = the `prev x cur` block of record f, rows = frame f); branch-free, a lane without a value reads a valid
    // address and keeps a zero
    auto load_b = [&](int e, bool first_of_sweep, bool with_image, double* xb) {
      const double* p = segc; int st = 0; bool ok = false;
      if (with_image) {
        if (role == 1 && first_of_sweep) {
          if (dir > 0) { p = segc + (size_t)a * kSegStride + kSegBpc + sub * 9; st = 1; ok = true; }                       // row `sub` of B_a
          else { ok = e + 1 < N; p = ok ? segc + (size_t)e * kSegStride + kSegBpc + sub : segc; st = ok ? 9 : 0; }        // column `sub` of B_e
        } else if (role == 3) {
          if (dir > 0) { ok = e + 1 < N; p = ok ? segc + (size_t)e * kSegStride + kSegBpc + sub : segc; st = ok ? 9 : 0; }
          else { p = segc + (size_t)(e - 1) * kSegStride + kSegBpc + sub * 9; st = 1; ok = true; }                          // row `sub` of B_{e-1}
        }
      }
      double y[9];
#pragma unroll
      for (int k = 0; k < 9; ++k) y[k] = p[k * st];
#pragma unroll
      for (int k = 0; k < 9; ++k) xb[k] = ok ? y[k] : 0.0;
    };
    auto take_img = [&](int e, bool with_image, double* x) {      // border and A columns, once the builder says so; added to the couplings
      if (!with_image) return;                                       // (wave-uniform)
      wait_ready(e - a);
      const double* im = IMG[e - a];
      if (role == 0 || role == 2) {
#pragma unroll
        for (int k = 0; k < 9; ++k) x[k] = im[k * kL0Ld + icol];
      }
    };
    double xin[9], o[9], dacc[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) { dacc[k] = 0.0; o[k] = 0.0; }
    {
      const int e = a + (cnt > 0 ? i0 : mid);
      const bool wi = cnt > 0 || wave == 0;
      load_b(e, true, wi, xin);
      take_img(e, wi, xin);
    }
    if (role == 2) {
#pragma unroll
      for (int k = 0; k < 9; ++k) An[k * 9 + sub] = xin[k];
    }
    // one elimination: A (in An) = L L^T, all columns solved, image stored, [X_s | X_n] to XS, out = [X_s | X_n]^T (column)
    const ElimLds elds = {XS, An, Ls};
    auto eliminate = [&](int e, double* x, double* out) { chain_eliminate<false>(v, v.cW + (size_t)e * isz, ldx, role, pc, sub, c == 0, elds, x, out); };
    for (int j = 0; ; ++j) {
      const bool at_mid = j == cnt;
      if (at_mid) {
        if (wave == 1) {
          if (cnt == 0) {
#pragma unroll
            for (int k = 0; k < 9; ++k) MID[k * W + c] = 0.0;
          }
#pragma unroll
          for (int k = 0; k < 9; ++k) SEPR[k * W + c] = dacc[k];
        }
        publish_sums();
        __syncthreads();                 // (all four wavefronts: the builders arrive when their frames are built)
        if (wave == 1) return;
#pragma unroll
        for (int k = 0; k < 9; ++k) {
          if (role == 0 || role == 2) xin[k] += MID[k * W + c];
          else if (role == 3 && nr > 0) xin[k] = MID[k * W + nW + sub];
        }
        if (role == 2) {
#pragma unroll
          for (int k = 0; k < 9; ++k) An[k * 9 + sub] = xin[k];
        }
      }
      const int e = a + (at_mid ? mid : i0 + dir * j);
      int en = 0; bool wn = false;
      if (!at_mid) {                      // the frame after this one: its couplings requested now, its image taken behind the elimination
        en = a + (j + 1 < cnt ? i0 + dir * (j + 1) : mid); wn = j + 1 < cnt || wave == 0;
        load_b(en, false, wn, o);
      }
      double x[9], out[18];
#pragma unroll
      for (int k = 0; k < 9; ++k) x[k] = xin[k];
      if (wv == 0) L0STAMP();               // sweep 0: frame taken, elimination starts
      eliminate(e, x, out);
      if (wv == 0) L0STAMP();               // ... and is done
#pragma unroll
      for (int k = 0; k < 9; ++k) dacc[k] += out[k];
      if (at_mid) {
        if (has_r && role < 4) {
          double* ri = v.rX[0] + (size_t)(r / 8) * isz + pc;
          const bool keep = role == 0 || role == 2;
          const int src = role == 2 ? nW + sub : c;
#pragma unroll
          for (int k = 0; k < 9; ++k) ri[k * ldx] = keep ? -out[9 + k] - SEPR[k * W + src] : 0.0;
        }
        if (role == 3) {
          double* img = v.cW + (size_t)a * isz + pc;
#pragma unroll
          for (int k = 0; k < 9; ++k) img[k * ldx] = has_r ? -out[k] : 0.0;
        }
        break;
      }
      if (wave == 1 && j + 1 == cnt) {
#pragma unroll
        for (int k = 0; k < 9; ++k) MID[k * W + c] = -out[9 + k];
      } else {
        take_img(en, wn, o);
#pragma unroll
        for (int k = 0; k < 9; ++k) xin[k] = o[k] - (role == 3 ? 0.0 : out[9 + k]);
        if (role == 2) {
#pragma unroll
          for (int k = 0; k < 9; ++k) An[k * 9 + sub] = xin[k];
        }
      }
    }
    // ---- the left separator absorbs its group: its border and A as builder 3 formed them, minus the group's update
    wait_ready(0);
    if (role == 0 || role == 1) {
      const int pcd = role == 1 ? ldw + 9 + sub : pc;
      double* img = v.cW + (size_t)a * isz + pcd;
#pragma unroll
      for (int k = 0; k < 9; ++k) img[k * ldx] = IMG[0][k * kL0Ld + icol] - dacc[k];
    }
#ifdef VC_L0_STAMPS
    __builtin_amdgcn_s_waitcnt(0);
    if (wv == 0) L0STAMP();
#endif
    return;
  }
  // ============================================================ the two builders: chunk sums ==========================================
  // ---- chunk sums (chunk = group): wavefronts 0, 1 (above) and builder 3 hand their sums over through LDS, builder 2 adds them to its own
  // in fixed order (2, 3, 0, 1) and writes the record
  __syncthreads();                       // (the sweeps' hand-over barrier: counts all four wavefronts)
  const int nsum = C * kGStride + kGStride;
  if (wv == 3) {
#pragma unroll
    for (int cc = 0; cc < CMAX; ++cc)
      if (cc < C) {
#pragma unroll
        for (int qq = 0; qq < 3; ++qq) {
          if (po[qq] >= 0) SUMW[3][cc * kGStride + po[qq]] = gsum[cc][qq];
          if (pm[qq] >= 0) SUMW[3][cc * kGStride + pm[qq]] = gsum[cc][qq];
        }
      }
#pragma unroll
    for (int qq = 0; qq < 4; ++qq) SUMW[3][C * kGStride + qq * 64 + lane] = isum[qq];
    if (lane < 9) SUMW[3][nsum + lane] = csum;
    set_ready(8 + 3);
    return;
  }
  // builder 2: its own sums through its (now free) Gram scratch, expanded like the others'
#pragma unroll
  for (int cc = 0; cc < CMAX; ++cc)
    if (cc < C) {
#pragma unroll
      for (int qq = 0; qq < 3; ++qq) {
        if (po[qq] >= 0) Gw[cc * kGStride + po[qq]] = gsum[cc][qq];
        if (pm[qq] >= 0) Gw[cc * kGStride + pm[qq]] = gsum[cc][qq];
      }
    }
  wave_lds_sync_local();
  wait_ready(8 + 3);
  const bool sw = q > 0;                  // (a group without interior frames: the sweeps built nothing and published nothing)
  if (sw) { wait_ready(8 + 0); wait_ready(8 + 1); }
  double* part = v.part + (size_t)group * v.part_stride;
  for (int e = lane; e < C * kGStride; e += 64) part[D * D + D + e] = ((Gw[e] + SUMW[3][e]) + (sw ? SUMW[0][e] : 0.0)) + (sw ? SUMW[1][e] : 0.0);
#pragma unroll
  for (int qq = 0; qq < 4; ++qq) {
    const int e = C * kGStride + qq * 64 + lane;
    part[D * D + D + e] = ((isum[qq] + SUMW[3][e]) + (sw ? SUMW[0][e] : 0.0)) + (sw ? SUMW[1][e] : 0.0);
  }
  for (int e = C * kGStride + 256 + lane; e < nsum; e += 64) part[D * D + D + e] = 0.0;
  {
    // fixed order: the nine lanes of builder 2, of builder 3, of wavefront 0, of wavefront 1
    const double t2 = (lane < 9) ? csum : 0.0, t3 = (lane < 9) ? SUMW[3][nsum + lane] : 0.0;
    const double t0 = (lane < 9 && sw) ? SUMW[0][nsum + lane] : 0.0, t1 = (lane < 9 && sw) ? SUMW[1][nsum + lane] : 0.0;
    double u2 = 0.0, u3 = 0.0, u0 = 0.0, u1 = 0.0;
#pragma unroll
    for (int kk = 0; kk < 9; ++kk) { u2 += readlane_f64(t2, kk); u3 += readlane_f64(t3, kk); u0 += readlane_f64(t0, kk); u1 += readlane_f64(t1, kk); }
    if (lane == 0) part[v.part_stride - 1] = ((u2 + u3) + u0) + u1;
  }
}

// Back-substitution of one level: delta_e = -L^-T (z + Y delta_s + X_s delta_a + X_n delta_next), right to left inside
// the group.  Everything that does not depend on the chain (z + Y delta_s + X_s delta_a, the rows of X_n, the columns of L)
// is formed by lane (frame i, row k) beforehand; the dependent part is one 9 x 9 product and a triangular solve per frame,
// exchanged through v_readlane.  At level 0 the wavefront also moves its frames (T <- T exp(delta), v <- v + dv) and
// publishes their step terms.
// phase stamps of one group of k_chain_back per level (profiling builds only: -DVC_BACK_STAMPS, tools/back_stamps.py): dbg[8 lvl + i]
#ifdef VC_BACK_STAMPS
#define BSTAMP(i) do { if (blockIdx.x == (top ? 0 : gridDim.x / 2) && threadIdx.x == 0 && lvl < 4) v.dbg[8 * lvl + (i)] = (long long)__builtin_amdgcn_s_memrealtime(); } while (0)
#else
#define BSTAMP(i) do { } while (0)
#endif
constexpr int kBackT0Frames = 1;      // frames per extra workgroup of the top-level launch (t0 = z + Y delta_s)
// FUSED: all levels below the top one in ONE launch (round 4).  A group needs the steps of its two separators, which a group of a
// level above produces: instead of a kernel boundary per level (four launches of ~9.5 us at cfg3 whose dependent chain is 2.5-3.6 us;
// the rest is launch, first loads and memory latency) every producer publishes its frames' steps with device-coherent stores and then
// raises the frames' ready words (the pass number), and a consumer -- which has requested everything else it needs beforehand --
// polls the two ready words and takes the steps with device-coherent loads: no fence, no cache write-back (the pattern of the
// cross-stream hand-overs).  Workgroups are laid out top level first: a group only ever waits for workgroups with a
// smaller index, which the dispatcher has started before it.
struct BackLevels { int n; int start[8]; int stride[8]; int m[8]; int two[8] /* 0 one sweep, 1 two sweeps, 2 odd-even */; };
// The dependent chain of a group that was eliminated odd-even (k_chain_oe, the top level; vc_chain_order.hpp): the last round first, every
// frame from its two neighbours of elimination time, y_i = t0_i + X_s,i d_left(i) + X_n,i d_right(i), L_i^T x = y_i, d_i = -x.  The frames of
// one round are independent chains of 9 x 9 products and triangular solves, interleaved instruction by instruction as the two sides of a
// two-sided group are.  lane = 9 fi + k: row k of interior frame fi + 1; t = t0 (WITHOUT the separator's term); da / dr: the separators'
// steps (zero where there is none).  The full group's order with compile-time indices, one slot per position 0 (a), 1 .. 7, 8 (r): frames
// beyond q stay zero, which is what "nobody on that side" means.
__device__ __forceinline__ double chain_back_oe(int q, int fi, int k, double t, const double* Xs, const double* Qrow, const double* Lcol, double dinv,
                                                const double* da, const double* dr) {
  double d[kOeMaxQ + 2][9];
#pragma unroll
  for (int j = 0; j < 9; ++j) {
    d[0][j] = da[j]; d[kOeMaxQ + 1][j] = dr[j];
#pragma unroll
    for (int i = 1; i <= kOeMaxQ; ++i) d[i][j] = 0.0;
  }
  double my = 0.0;
#pragma unroll
  for (int st = kOeMaxSteps; st >= 1; --st) {
    const int h = 1 << (st - 1);                                // the round's frames: h, 3 h, 5 h, .. (up to four)
    if (h <= q) {                                               // (wave-uniform)
      double y[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int i = h * (2 * u + 1);
        y[u] = t;
        if (i <= kOeMaxQ) {
          const OeFrame f = oe_full(i);
#pragma unroll
          for (int c = 0; c < 9; ++c) y[u] += Xs[c] * d[oe_slot(f.left)][c] + Qrow[c] * d[oe_slot(f.right)][c];
        }
      }
#pragma unroll
      for (int j = 8; j >= 0; --j) {
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          const int i = h * (2 * u + 1);
          if (i <= kOeMaxQ) {
            const double xj = readlane_f64(y[u] * dinv, (i - 1) * 9 + j);
            if (i <= q) { d[i][j] = -xj; y[u] -= Lcol[j] * xj; }
          }
        }
      }
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int i = h * (2 * u + 1);
        if (i <= kOeMaxQ && i <= q && fi == i - 1) {
#pragma unroll
          for (int j = 0; j < 9; ++j) my = (j == k) ? d[i][j] : my;
        }
      }
    }
  }
  return my;
}
template <bool FUSED>
__device__ __forceinline__ void chain_back_group(const DevView& v, int s, int m, int top, int lvl, int two, int group, double* ds, double* dl) {
  const int done = v.ctrl->done;        // looked at once the level's inputs have been requested (see k_chain_fwd)
  const int lane = threadIdx.x;
#ifdef VC_BACK_STAMPS
  const long long bs0_ = (long long)__builtin_amdgcn_s_memrealtime();
#endif
  const int N = v.n_frames, D = v.D, ldw = v.ldw, ldx = v.ldx;
  const long gs = (long)m * s;
  const int a = top ? -1 : (int)(group * gs);
  const int first = top ? 0 : a + s;
  const size_t isz = (size_t)9 * ldx;
  for (int j = lane; j < D; j += 64) ds[j] = v.delta_s[j];
  const int q = first < N ? (top ? (N - 1) / s + 1 : min(m - 1, (N - 1 - first) / s + 1)) : 0;
  const int r = first + q * s;                                  // right separator (or past the end)
  double da[9], dn[9];
  const bool has_a = a >= 0 && a < N, has_r = !top && q > 0 && r < N;
  if (!FUSED) {
#pragma unroll
    for (int k = 0; k < 9; ++k) { da[k] = has_a ? v.cdelta[(size_t)a * 9 + k] : 0.0; dn[k] = has_r ? v.cdelta[(size_t)r * 9 + k] : 0.0; }
  }
  const int fi = lane / 9, k = lane % 9;
  const bool mine = fi < q;
  const int e = first + (mine ? fi : 0) * s;
  // a group eliminated from both ends (k_chain_fwd2: full groups of a level launched two-sided): frames right of the middle hang
  // on the right separator and on the frame to their left
  const bool two_sided = two == 1 && !top && q >= 1;
  const bool oe = two == 2;                                      // eliminated odd-even (k_chain_oe / the top level): chain_back_oe
  const int fmid = (q - 1) / 2;                                  // lane group of the middle frame (interior index fmid + 1)
  double t = 0.0, dinv = 1.0, Qrow[9], Lcol[9];
#pragma unroll
  for (int c = 0; c < 9; ++c) { Qrow[c] = 0.0; Lcol[c] = 0.0; }
  if (top) wave_lds_sync();      // (the levels below need delta_s only in the bottom level's epilogue, behind its own synchronisation)
#ifdef VC_BACK_STAMPS
  const long long bs1_ = (long long)__builtin_amdgcn_s_memrealtime();
#endif
  if (mine) {
    const double* img = v.cW + (size_t)e * isz;
    const double* Wr = img + (size_t)k * ldx;
#pragma unroll
    for (int c = 0; c < 9; ++c) { Qrow[c] = Wr[ldw + 18 + c]; Lcol[c] = (c > k) ? img[c * ldx + ldw + 9 + k] : 0.0; }
    dinv = 1.0 / Wr[ldw + 9 + k];
    double acc;
    if (top) { acc = Wr[D]; for (int j = 0; j < D; ++j) acc += Wr[j] * ds[j]; }      // (its own frames: the extra workgroups run beside it)
    else acc = v.ct0[(size_t)e * 9 + k];
    t = acc;
  }
  double Xs[9];
#pragma unroll
  for (int c = 0; c < 9; ++c) Xs[c] = (mine && (a >= 0 || oe)) ? v.cW[(size_t)e * isz + (size_t)k * ldx + ldw + c] : 0.0;      // (oe: the left NEIGHBOUR's coupling, the top level's frames too)
  if (done) return;
  if (FUSED) {
    // everything else is on its way: now the separators' steps (the levels above publish them, see the kernel's header)
    if (lane == 0) {
      long long n = 0;
      while ((has_a && __hip_atomic_load(v.cready + a, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < v.pass_id) ||
             (has_r && __hip_atomic_load(v.cready + r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < v.pass_id)) {
        __builtin_amdgcn_s_sleep(2);
        // (never seen: would take a dispatcher that starts workgroups out of order.  Loud and lossless like the cross-stream waits where a
        //  resume exists -- the pass is marked void, the host reports it and repeats the pass with events; a numeric-failure mark otherwise)
        if (++n > 4000000) {
          if (v.sync_seq > 0) mark_sync_timeout(v, v.sync_seq); else atomicAdd(&v.flags[4 + 2 * v.par], 1);
          atomicAdd((unsigned long long*)&v.dbg[21], 1ull);
          break;
        }
      }
    }
    __builtin_amdgcn_wave_barrier();
    (void)__builtin_amdgcn_readfirstlane(lane);      // (the wavefront goes on together)
#pragma unroll
    for (int k2 = 0; k2 < 9; ++k2) {
      da[k2] = has_a ? __hip_atomic_load(v.cdelta + (size_t)a * 9 + k2, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0.0;
      dn[k2] = has_r ? __hip_atomic_load(v.cdelta + (size_t)r * 9 + k2, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0.0;
    }
  }
  if (mine && a >= 0 && !oe) {
    const bool right = two_sided && fi > fmid;
#pragma unroll
    for (int c = 0; c < 9; ++c) t += Xs[c] * (right ? dn[c] : da[c]);       // (dn: still the right separator's step here)
  }
#ifdef VC_BACK_STAMPS
  if (__builtin_amdgcn_readfirstlane(__double2loint(t)) == 0x7fffffff) return;      // (forces t before the stamp)
  if (blockIdx.x == (top ? 0 : gridDim.x / 2) && threadIdx.x == 0 && lvl < 4) { v.dbg[8 * lvl] = bs0_; v.dbg[8 * lvl + 1] = bs1_; }      // (not in passes that exit early)
#endif
  BSTAMP(2);
  double my = 0.0;
  if (oe) my = chain_back_oe(q, fi, k, t, Xs, Qrow, Lcol, dinv, da, dn);
  else if (two_sided) {
    // the middle first (a on its left, r on its right), then outwards on both sides at once: two independent chains of 9 x 9
    // products and triangular solves, interleaved instruction by instruction
    {
      double y = t;
#pragma unroll
      for (int c = 0; c < 9; ++c) y += Qrow[c] * dn[c];
#pragma unroll
      for (int j = 8; j >= 0; --j) {
        const double xj = readlane_f64(y * dinv, fmid * 9 + j);
        dn[j] = -xj;
        y -= Lcol[j] * xj;
      }
      if (fi == fmid) {
#pragma unroll
        for (int j = 0; j < 9; ++j) my = (j == k) ? dn[j] : my;
      }
    }
    double dl_[9], dr_[9];
#pragma unroll
    for (int j = 0; j < 9; ++j) { dl_[j] = dn[j]; dr_[j] = dn[j]; }
    const int nleft = fmid, nright = q - 1 - fmid;
    for (int st = 1; st <= max(nleft, nright); ++st) {
      const bool hl = st <= nleft, hr = st <= nright;              // wave-uniform
      const int il = hl ? fmid - st : 0, ir = hr ? fmid + st : 0;
      double yl = t, yr = t;
#pragma unroll
      for (int c = 0; c < 9; ++c) { yl += Qrow[c] * dl_[c]; yr += Qrow[c] * dr_[c]; }
#pragma unroll
      for (int j = 8; j >= 0; --j) {
        const double xl = readlane_f64(yl * dinv, il * 9 + j), xr = readlane_f64(yr * dinv, ir * 9 + j);
        if (hl) { dl_[j] = -xl; yl -= Lcol[j] * xl; }
        if (hr) { dr_[j] = -xr; yr -= Lcol[j] * xr; }
      }
      if (hl && fi == il) {
#pragma unroll
        for (int j = 0; j < 9; ++j) my = (j == k) ? dl_[j] : my;
      }
      if (hr && fi == ir) {
#pragma unroll
        for (int j = 0; j < 9; ++j) my = (j == k) ? dr_[j] : my;
      }
    }
  } else
  for (int i = q - 1; i >= 0; --i) {
    double y = t;
#pragma unroll
    for (int c = 0; c < 9; ++c) y += Qrow[c] * dn[c];
#pragma unroll
    for (int j = 8; j >= 0; --j) {
      const double xj = readlane_f64(y * dinv, i * 9 + j);
      dn[j] = -xj;
      y -= Lcol[j] * xj;
    }
    if (fi == i) {
#pragma unroll
      for (int j = 0; j < 9; ++j) my = (j == k) ? dn[j] : my;
    }
  }
#ifdef VC_BACK_STAMPS
  if (__builtin_amdgcn_readfirstlane(__double2loint(my)) == 0x7fffffff) return;
#endif
  BSTAMP(3);
  if (lvl != 0 && v.cready) {
    // frames of this level are separators of the levels below: device-coherent stores, then -- once the wavefront's stores have
    // been performed -- the frames' ready words
    if (mine) __hip_atomic_store(v.cdelta + (size_t)e * 9 + k, my, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __builtin_amdgcn_s_waitcnt(0);
    __builtin_amdgcn_wave_barrier();
    if (mine && k == 0) __hip_atomic_store(v.cready + e, v.pass_id, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  } else if (mine) v.cdelta[(size_t)e * 9 + k] = my;
  if (lvl != 0) { BSTAMP(4); return; }
  // ---- level 0: trial poses / velocities of the group's frames and their step terms
  if (mine) dl[(fi + 1) * 9 + k] = my;
  if (lane < 9) dl[lane] = da[lane];
  wave_lds_sync();
  const int base = top ? 0 : a, cnt = top ? q : (a < N ? q + 1 : 0), off = top ? 1 : 0;
  double gd = 0, dld = 0, step2 = 0, x2 = 0, g2 = 0, gmax = 0;
  if (lane < cnt) {
    const int f = base + lane;
    const int cur = v.ctrl->cur;
    // pinned frames step with the reduced system's solution; their gradient / damping terms are counted there, and only the
    // owner (not the rank that holds the ghost copy) counts the step and parameter norms
    const bool pin_f = (f == 0 && v.pin_first), pin_l = (f == N - 1 && v.pin_last);
    double d[9];
#pragma unroll
    for (int i = 0; i < 9; ++i) d[i] = pin_f ? ds[v.sep_col0 + i] : pin_l ? ds[v.sep_col1 + i] : dl[(lane + off) * 9 + i];
    const double* pin = v.poses[cur] + (size_t)f * kPoseStride;
    double* pout = v.poses[1 - cur] + (size_t)f * kPoseStride;
    double Tin[7], Tout[7], dd[6];
    for (int i = 0; i < 7; ++i) Tin[i] = pin[i];
    for (int i = 0; i < 6; ++i) dd[i] = d[i];
    se3_plus(Tin, dd, Tout);
    for (int i = 0; i < 7; ++i) { pout[i] = Tout[i]; const double ee = Tout[i] - Tin[i]; step2 += ee * ee; x2 += Tin[i] * Tin[i]; }
    pout[7] = 0.0;
    const double* vin = v.vel[cur] + (size_t)f * 4;
    double* vout = v.vel[1 - cur] + (size_t)f * 4;
    for (int i = 0; i < 3; ++i) { const double dv = d[6 + i]; vout[i] = vin[i] + dv; step2 += dv * dv; x2 += vin[i] * vin[i]; }
    vout[3] = 0.0;
    for (int i = 0; i < 9; ++i) {
      const double gi = v.cg[(size_t)f * 9 + i];
      gd += gi * d[i]; dld += v.clam[(size_t)f * 9 + i] * d[i] * d[i]; g2 += gi * gi; gmax = fmax(gmax, fabs(gi));
    }
    if (pin_f || pin_l) { gd = 0; dld = 0; g2 = 0; gmax = 0; }
    if (pin_l) { step2 = 0; x2 = 0; }
  }
  // the group's step terms in one record (lanes >= cnt hold zeros; fixed summation order)
  gd = wave_sum(gd); dld = wave_sum(dld); step2 = wave_sum(step2); x2 = wave_sum(x2); g2 = wave_sum(g2);
#pragma unroll
  for (int o2 = 32; o2 > 0; o2 >>= 1) gmax = fmax(gmax, __shfl_down(gmax, o2, 64));
  if (lane == 0) {
    double* o = v.grp_part + (size_t)group * kNumScal;
    o[kScGd] = gd; o[kScDld] = dld; o[kScStep2] = step2; o[kScX2] = x2; o[kScG2] = g2; o[kScCost] = 0.0; o[kScGmax] = gmax; o[kScSq] = 0.0;
  }
  BSTAMP(4);
}

__global__ __launch_bounds__(64) void k_chain_back(DevView v, int s, int m, int top, int lvl, int two) {
  __shared__ double ds[192 + 8];
  __shared__ double dl[kChainM * 9];
  const int lane = threadIdx.x;
  const int D = v.D, ldx = v.ldx;
  const size_t isz = (size_t)9 * ldx;
  // The chain-independent part of every right-hand side, t0 = z + Y delta_s, for ALL frames: extra workgroups of the top level's
  // launch (which has one group and an idle chip beside it), lane = column so that a load instruction covers one row segment --
  // the levels below read one value per (frame, row) instead of walking D entries of a row per lane, 63 cache lines per load
  // instruction (2.5 us per level at D = 29, 7-16 us at D = 115; tools/back_stamps.py).
  if (top && blockIdx.x > 0) {
    if (v.ctrl->done) return;
    const int f = (int)blockIdx.x - 1;      // one frame per wavefront: its nine rows' loads go out together
    double dsl[3];
#pragma unroll
    for (int u = 0; u < 3; ++u) { const int j = lane + 64 * u; dsl[u] = j < D ? v.delta_s[j] : (j == D ? 1.0 : 0.0); }      // (column D: z itself)
    double p[9];
#pragma unroll
    for (int kk = 0; kk < 9; ++kk) {
      const double* Wr = v.cW + (size_t)f * isz + (size_t)kk * ldx;
      double acc = 0.0;
#pragma unroll
      for (int w = 0; w < 3; ++w) { const int j = lane + 64 * w; if (j <= D) acc += Wr[j] * dsl[w]; }
      p[kk] = acc;
    }
#pragma unroll
    for (int kk = 0; kk < 9; ++kk) {
      const double t0 = wave_sum(p[kk]);
      if (lane == 0) v.ct0[(size_t)f * 9 + kk] = t0;
    }
    return;
  }
  chain_back_group<false>(v, s, m, top, lvl, two, (int)blockIdx.x, ds, dl);
}
// ... the same sums as a launch of their own, one frame per wavefront: what the one-launch back-substitution reads at wide borders
// (k_chain_back_path below recomputes the upper levels in every bottom group -- with their rows [Y | z] that is 58 KB per wavefront at
// D = 115, 230 MB through the L2 at 6250 frames: the one-launch form then took 218 us against 71 for the level-by-level kernels; with t0
// formed once per frame here it reads nine values per frame)
__global__ __launch_bounds__(256) void k_chain_t0(DevView v) {
  if (v.ctrl->done) return;
  const int lane = threadIdx.x & 63, f = (int)blockIdx.x * 4 + (int)(threadIdx.x >> 6);
  if (f >= v.n_frames) return;
  const int D = v.D, ldx = v.ldx;
  double dsl[3];
#pragma unroll
  for (int u = 0; u < 3; ++u) { const int j = lane + 64 * u; dsl[u] = j < D ? v.delta_s[j] : (j == D ? 1.0 : 0.0); }      // (column D: z itself)
  double p[9];
#pragma unroll
  for (int kk = 0; kk < 9; ++kk) {
    const double* Wr = v.cW + ((size_t)f * 9 + kk) * ldx;
    double x[3];
#pragma unroll
    for (int w = 0; w < 3; ++w) { const int j = lane + 64 * w; x[w] = Wr[j <= D ? j : 0]; }
    double acc = 0.0;
#pragma unroll
    for (int w = 0; w < 3; ++w) { const int j = lane + 64 * w; acc += (j <= D) ? x[w] * dsl[w] : 0.0; }
    p[kk] = acc;
  }
#pragma unroll
  for (int kk = 0; kk < 9; ++kk) {
    const double t0 = wave_sum(p[kk]);
    if (lane == 0) v.ct0[(size_t)f * 9 + kk] = t0;
  }
}
__global__ __launch_bounds__(64) void k_chain_back_levels(DevView v, BackLevels L) {
  __shared__ double ds[192 + 8];
  __shared__ double dl[kChainM * 9];
  int li = 0;
#pragma unroll
  for (int i = 1; i < 8; ++i) if (i < L.n && (int)blockIdx.x >= L.start[i]) li = i;
  const int lvl = L.n - 1 - li;                       // (the table runs from the highest level down to level 0)
  chain_back_group<true>(v, L.stride[li], L.m[li], 0, lvl, L.two[li], (int)blockIdx.x - L.start[li], ds, dl);
}

// PATH (round 5): the whole back-substitution in ONE launch without any hand-over between workgroups.  A workgroup per bottom-level
// group; wavefront w works the group of level w that the bottom group hangs under (the last wavefront: the top level) -- the upper
// levels are recomputed by every workgroup below them (8 / 64 / 250 times at cfg3: a few hundred KB more of L2 reads) instead of being
// handed down through device-coherent stores and ready words (~5.5 us per level) or kernel boundaries.  All wavefronts request their
// group's data at once; t0 = z + Y delta_s of the group's frames is formed in the kernel (rows staged through LDS: coalesced loads,
// then one row per lane) -- the extra workgroups of the top level's launch and the ct0 round trip are gone with the launch; the steps
// travel top-down through LDS (positions of a group: 0 = left separator, 1 .. q = interior frames, q + 1 = right separator; the top
// level: its frames from position 0).  The dependent chain is chain_back_group's, instruction for instruction.
// Round 6: any border width and sharded passes.  Borders of more than kPathRowCols columns take t0 from k_chain_t0 (instance CT0: staging
// the rows of the recomputed levels in every bottom group then costs more than a launch -- measured 218 us against 71 for the level-by-level
// kernels at 6250 frames x D = 115, 120 us with t0 from its own launch); a pinned frame (separator / ghost of a sharded chain,
// DevView::pin_first / pin_last) steps with the reduced system's solution in the epilogue.
struct BackPath { int n; int stride[6]; int m[6]; int two[6] /* 0 one sweep, 1 two sweeps, 2 odd-even */; int oe_top; int top_stride; int ldr; int dsw; int tail; };
// (round 6) the launch's LAST workgroup, when BackPath::tail is set, is not a bottom group: it forms what k_reduced left out
// (DevView::tail_deferred) -- the trial cameras and the shared parameters' terms of the step scalars -- beside the back-substitution
// instead of at the end of a one-workgroup kernel the whole chip waits for.  The first 256 threads; LDS: kTailLds doubles.
constexpr int kTailLds = kMaxCams * kCamStride + 16 + 8 + 6 * 256;
__device__ __forceinline__ void reduced_tail_workgroup(const DevView& v, double* lds) {
  const int tid = threadIdx.x, D = v.D;
  if (tid >= 256) return;
  const Ctrl* ct = v.ctrl;
  const int cur = ct->cur, done = ct->done;
  if (done) return;
  double* s_cam = lds;
  CamDesc* s_cd = reinterpret_cast<CamDesc*>(lds + kMaxCams * kCamStride);
  int* s_ipc = reinterpret_cast<int*>(lds + kMaxCams * kCamStride + 16);
  double* red = lds + kMaxCams * kCamStride + 16 + 8;
  for (int i = tid; i < v.n_cams * kCamStride; i += 256) s_cam[i] = v.cams[cur][i];
  if (tid < kMaxCams) s_cd[tid] = v.cd[tid];
  if (tid >= 64 && tid < 64 + 15) s_ipc[tid - 64] = v.imu_param_col[tid - 64];
  double pre_imu = 0.0;
  if (v.imu_on && (tid >> 6) == (D <= 64 ? 0 : 1) && (tid & 63) < 16) pre_imu = v.imus[cur][tid & 63];
  __syncthreads();
  reduced_tail(v, cur, v.delta_s, v.Sbuf + (size_t)D * D + 2 * D, v.slam, s_cam, s_cd, s_ipc, pre_imu, nullptr, red, false, false);
}
constexpr int kPathRowCols = 37;       // widest row [Y | z] the in-kernel staging serves (D + 1 entries)
constexpr int kPathRowLoads = 37;      // 63 rows x kPathRowCols entries over 64 lanes
constexpr int kPathDl = 96;            // doubles per level's step record (10 positions x 9)
template <int NWMAX, bool CT0>      // wavefronts per workgroup at most (levels + 1): up to four leave a whole SIMD's registers to each; CT0: t0 from k_chain_t0
#ifdef VC_BACK_PATH_EU      // (A/B builds, as VC_IMU_BLOCK_EU: n = 3: 168 registers, 212 B of scratch)
__global__ __launch_bounds__(64 * NWMAX) __attribute__((amdgpu_waves_per_eu(VC_BACK_PATH_EU, VC_BACK_PATH_EU))) void k_chain_back_path(DevView v, BackPath P) {
#else
__global__ __launch_bounds__(64 * NWMAX) void k_chain_back_path(DevView v, BackPath P) {
#endif
  extern __shared__ __attribute__((aligned(16))) double bp_lds[];
  if (P.tail && blockIdx.x == gridDim.x - 1) { reduced_tail_workgroup(v, bp_lds); return; }
  const int wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), lane = threadIdx.x & 63;
  const int nw = P.n + 1;
  double* DLall = bp_lds;                              // [nw][kPathDl]
  double* DSW = DLall + nw * kPathDl + (size_t)wv * P.dsw;      // this wavefront's copy of delta_s
  int* READY = reinterpret_cast<int*>(DLall + nw * kPathDl + nw * P.dsw);      // [8]
  double* RW = DLall + nw * kPathDl + nw * P.dsw + 4 + (size_t)wv * 63 * P.ldr;      // this wavefront's rows [63][ldr]
  double* DL = DLall + (size_t)wv * kPathDl;
  if (threadIdx.x < 8) READY[threadIdx.x] = 0;
  __syncthreads();
  auto wait_ready = [&](int slot) {
    while (__hip_atomic_load(&READY[slot], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) == 0) __builtin_amdgcn_s_sleep(1);
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    __builtin_amdgcn_wave_barrier();
  };
  auto set_ready = [&](int slot) {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_s_waitcnt(0xc07f);          // lgkmcnt(0): this wavefront's LDS stores have been performed
    __builtin_amdgcn_wave_barrier();
    if (lane == 0) __hip_atomic_store(&READY[slot], 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
  };
  const int done = v.ctrl->done;
  const int N = v.n_frames, D = v.D, ldw = v.ldw, ldx = v.ldx;
  const size_t isz = (size_t)9 * ldx;
  const bool top = wv == P.n;
  const int lvl = top ? P.n : wv;
  const int s = top ? P.top_stride : P.stride[lvl], m = top ? kChainM : P.m[lvl], two = top ? (P.oe_top ? 2 : 0) : P.two[lvl];
  const long gs = (long)m * s;
  const long a0 = (long)blockIdx.x * P.m[0] * P.stride[0];        // the bottom group's left separator
  const int a = top ? -1 : (int)((a0 / gs) * gs);
  const int first = top ? 0 : a + s;
  const int q = first < N ? (top ? (N - 1) / s + 1 : min(m - 1, (N - 1 - first) / s + 1)) : 0;
  const int r = first + q * s;
  const bool has_a = a >= 0 && a < N, has_r = !top && q > 0 && r < N;
  const int fi = lane / 9, k = lane % 9;
  const bool mine = fi < q;
  const int e = first + (mine ? fi : 0) * s;
  const bool two_sided = two == 1 && !top && q >= 1;
  const bool oe = two == 2;
  const int fmid = (q - 1) / 2;
  // ---- requests: the rows [Y | z] of the group's frames (lane-strided, coalesced; narrow borders only -- CT0: t0 comes finished from
  // k_chain_t0), then this lane's blocks
  const int ncolr = D + 1, nel = q * 9 * ncolr;
  double rv[CT0 ? 1 : kPathRowLoads];
  if (!CT0) {
    const int step_r = 64 / ncolr, step_c = 64 - step_r * ncolr;
    int row = lane / ncolr, col = lane - row * ncolr;
#pragma unroll
    for (int u = 0; u < kPathRowLoads; ++u) {
      const int idx = lane + 64 * u;
      const int f2 = (row * 57) >> 9, k2 = row - 9 * f2;          // (row / 9 for rows below 64)
      const bool in = idx < nel;          // (a lane without an entry reads frame 0 and drops the value)
      const double* src = v.cW + (size_t)(in ? first + f2 * s : 0) * isz + (size_t)(in ? k2 : 0) * ldx + (in ? col : 0);
      const double x = *src;
      rv[u] = in ? x : 0.0;
      row += step_r; col += step_c;
      if (col >= ncolr) { col -= ncolr; ++row; }
    }
  }
  double dsv[3];
#pragma unroll
  for (int u = 0; u < (CT0 ? 3 : 1); ++u) { const int j = lane + 64 * u; dsv[u] = v.delta_s[j < D ? j : 0]; }
  double dinv = 1.0, Qrow[9], Lcol[9], Xs[9], t0_in = 0.0;
  {
    const double* img = v.cW + (size_t)(mine ? e : 0) * isz;
    const double* Wr = img + (size_t)k * ldx;
#pragma unroll
    for (int c = 0; c < 9; ++c) {
      const double qv = Wr[ldw + 18 + c], lv = img[c * ldx + ldw + 9 + k], xv = Wr[ldw + c];
      Qrow[c] = mine ? qv : 0.0; Lcol[c] = (mine && c > k) ? lv : 0.0; Xs[c] = (mine && (a >= 0 || oe)) ? xv : 0.0;
    }
    const double dg = Wr[ldw + 9 + k];
    dinv = mine ? 1.0 / dg : 1.0;
    if (CT0) { const double tv = v.ct0[(size_t)(mine ? e : 0) * 9 + k]; t0_in = mine ? tv : 0.0; }      // (the finished sum z + Y delta_s)
  }
  const int base = a, cnt = (a < N) ? q + 1 : 0;
  if (done) return;                      // (uniform over the workgroup)
#pragma unroll
  for (int u = 0; u < (CT0 ? 3 : 1); ++u) { const int j = lane + 64 * u; if (j < D) DSW[j] = dsv[u]; }
  double t = t0_in;
  if (!CT0) {
    int row = lane / ncolr, col = lane - row * ncolr;
    const int step_r = 64 / ncolr, step_c = 64 - step_r * ncolr;
#pragma unroll
    for (int u = 0; u < kPathRowLoads; ++u) {
      const int idx = lane + 64 * u;
      if (idx < nel) RW[row * P.ldr + col] = rv[u];
      row += step_r; col += step_c;
      if (col >= ncolr) { col -= ncolr; ++row; }
    }
    wave_lds_sync_local();
    if (mine) {
      const double* Rr = RW + (size_t)(fi * 9 + k) * P.ldr;
      double acc = Rr[D];
      for (int j = 0; j < D; ++j) acc += Rr[j] * DSW[j];
      t = acc;
    }
  }
  // ---- the separators' steps from the level above
  double da[9], dn[9], dr_in[9];
#pragma unroll
  for (int c = 0; c < 9; ++c) { da[c] = 0.0; dn[c] = 0.0; }
  if (!top) {
    wait_ready(lvl + 1);
    const double* DLp = DLall + (size_t)(lvl + 1) * kPathDl;
    int pos;
    if (lvl + 1 == P.n) pos = a / P.top_stride;                               // the top level keeps its frames from position 0
    else { const long gp = (long)P.m[lvl + 1] * P.stride[lvl + 1]; const int ap = (int)((a0 / gp) * gp); pos = (a - ap) / P.stride[lvl + 1]; }
#pragma unroll
    for (int c = 0; c < 9; ++c) {
      const double x0 = DLp[pos * 9 + c], x1 = DLp[(pos + 1) * 9 + c];
      da[c] = has_a ? x0 : 0.0; dn[c] = has_r ? x1 : 0.0;
    }
  }
#pragma unroll
  for (int c = 0; c < 9; ++c) dr_in[c] = dn[c];
  if (mine && a >= 0 && !oe) {
    const bool right = two_sided && fi > fmid;
#pragma unroll
    for (int c = 0; c < 9; ++c) t += Xs[c] * (right ? dn[c] : da[c]);       // (dn: still the right separator's step here)
  }
  double my = 0.0;
  if (oe) my = chain_back_oe(q, fi, k, t, Xs, Qrow, Lcol, dinv, da, dn);
  else if (two_sided) {
    {
      double y = t;
#pragma unroll
      for (int c = 0; c < 9; ++c) y += Qrow[c] * dn[c];
#pragma unroll
      for (int j = 8; j >= 0; --j) {
        const double xj = readlane_f64(y * dinv, fmid * 9 + j);
        dn[j] = -xj;
        y -= Lcol[j] * xj;
      }
      if (fi == fmid) {
#pragma unroll
        for (int j = 0; j < 9; ++j) my = (j == k) ? dn[j] : my;
      }
    }
    double dl_[9], dr_[9];
#pragma unroll
    for (int j = 0; j < 9; ++j) { dl_[j] = dn[j]; dr_[j] = dn[j]; }
    const int nleft = fmid, nright = q - 1 - fmid;
    for (int st = 1; st <= max(nleft, nright); ++st) {
      const bool hl = st <= nleft, hr = st <= nright;              // wave-uniform
      const int il = hl ? fmid - st : 0, ir = hr ? fmid + st : 0;
      double yl = t, yr = t;
#pragma unroll
      for (int c = 0; c < 9; ++c) { yl += Qrow[c] * dl_[c]; yr += Qrow[c] * dr_[c]; }
#pragma unroll
      for (int j = 8; j >= 0; --j) {
        const double xl = readlane_f64(yl * dinv, il * 9 + j), xr = readlane_f64(yr * dinv, ir * 9 + j);
        if (hl) { dl_[j] = -xl; yl -= Lcol[j] * xl; }
        if (hr) { dr_[j] = -xr; yr -= Lcol[j] * xr; }
      }
      if (hl && fi == il) {
#pragma unroll
        for (int j = 0; j < 9; ++j) my = (j == k) ? dl_[j] : my;
      }
      if (hr && fi == ir) {
#pragma unroll
        for (int j = 0; j < 9; ++j) my = (j == k) ? dr_[j] : my;
      }
    }
  } else
  for (int i = q - 1; i >= 0; --i) {
    double y = t;
#pragma unroll
    for (int c = 0; c < 9; ++c) y += Qrow[c] * dn[c];
#pragma unroll
    for (int j = 8; j >= 0; --j) {
      const double xj = readlane_f64(y * dinv, i * 9 + j);
      dn[j] = -xj;
      y -= Lcol[j] * xj;
    }
    if (fi == i) {
#pragma unroll
      for (int j = 0; j < 9; ++j) my = (j == k) ? dn[j] : my;
    }
  }
  // ---- this level's steps for the level below (the bottom level: for its own epilogue)
  if (mine) DL[(fi + (top ? 0 : 1)) * 9 + k] = my;
  if (!top && lane < 9) { DL[lane] = da[lane]; DL[(q + 1) * 9 + lane] = dr_in[lane]; }
  if (lvl != 0 || top) { set_ready(lvl); return; }
  wave_lds_sync_local();
  // ---- level 0: trial poses / velocities of the group's frames and their step terms (chain_back_group's epilogue)
  double gd = 0, dld = 0, step2 = 0, x2 = 0, g2 = 0, gmax = 0;
  if (lane < cnt) {
    const int f = base + lane;
    const int cur = v.ctrl->cur;
    double d[9], Tin[7], vin[3], gi9[9], lam9[9];
    {
      const double* pin = v.poses[cur] + (size_t)f * kPoseStride;
      const double* vi = v.vel[cur] + (size_t)f * 4;
#pragma unroll
      for (int i = 0; i < 7; ++i) Tin[i] = pin[i];
#pragma unroll
      for (int i = 0; i < 3; ++i) vin[i] = vi[i];
#pragma unroll
      for (int i = 0; i < 9; ++i) { gi9[i] = v.cg[(size_t)f * 9 + i]; lam9[i] = v.clam[(size_t)f * 9 + i]; }
    }
    // pinned frames (sharded chain) step with the reduced system's solution; their gradient / damping terms are counted there, and only
    // the owner (not the rank that holds the ghost copy) counts the step and parameter norms -- chain_back_group's rule
    const bool pin_f = (f == 0 && v.pin_first), pin_l = (f == N - 1 && v.pin_last);
    const int sc = pin_f ? v.sep_col0 : (pin_l ? v.sep_col1 : 0);
#pragma unroll
    for (int i = 0; i < 9; ++i) { const double dch = DL[lane * 9 + i], dsp = DSW[sc + i]; d[i] = (pin_f || pin_l) ? dsp : dch; }
    double* pout = v.poses[1 - cur] + (size_t)f * kPoseStride;
    double Tout[7], dd[6];
    for (int i = 0; i < 6; ++i) dd[i] = d[i];
    se3_plus(Tin, dd, Tout);
    for (int i = 0; i < 7; ++i) { pout[i] = Tout[i]; const double ee = Tout[i] - Tin[i]; step2 += ee * ee; x2 += Tin[i] * Tin[i]; }
    pout[7] = 0.0;
    double* vout = v.vel[1 - cur] + (size_t)f * 4;
    for (int i = 0; i < 3; ++i) { const double dv = d[6 + i]; vout[i] = vin[i] + dv; step2 += dv * dv; x2 += vin[i] * vin[i]; }
    vout[3] = 0.0;
    for (int i = 0; i < 9; ++i) {
      const double gi = gi9[i];
      gd += gi * d[i]; dld += lam9[i] * d[i] * d[i]; g2 += gi * gi; gmax = fmax(gmax, fabs(gi));
    }
    if (pin_f || pin_l) { gd = 0; dld = 0; g2 = 0; gmax = 0; }
    if (pin_l) { step2 = 0; x2 = 0; }
  }
  gd = wave_sum(gd); dld = wave_sum(dld); step2 = wave_sum(step2); x2 = wave_sum(x2); g2 = wave_sum(g2);
#pragma unroll
  for (int o2 = 32; o2 > 0; o2 >>= 1) gmax = fmax(gmax, __shfl_down(gmax, o2, 64));
  if (lane == 0) {
    double* o = v.grp_part + (size_t)blockIdx.x * kNumScal;
    o[kScGd] = gd; o[kScDld] = dld; o[kScStep2] = step2; o[kScX2] = x2; o[kScG2] = g2; o[kScCost] = 0.0; o[kScGmax] = gmax; o[kScSq] = 0.0;
  }
}

// sum over all frames of [Y | z]^T [Y | z]: part[chunk] = [ D x D | D ]  (same layout as the vision path)
constexpr int kMaxPairsPerWaveI = 9;
// phase stamps of one workgroup of k_chain_gram (profiling builds only: -DVC_GRAM_STAMPS, tools/gram_stamps.py)
#ifdef VC_GRAM_STAMPS
#define GSTAMP(i) do { if (blockIdx.x == gridDim.x / 2 && threadIdx.x == 0 && (i) < 16) v.dbg[i] = (long long)__builtin_amdgcn_s_memrealtime(); } while (0)
#else
#define GSTAMP(i) do { } while (0)
#endif
// NQ: column-tile pairs per wavefront and batch (accumulators with compile-time indices: the version that picked its accumulator
// with a runtime index spent ~150 v_cndmask per pair on it and ran the nine MFMAs of a pair as one dependent chain -- 7.8 us per
// group of four frames at D = 115; here the NQ chains advance side by side).  Rows of the next group are requested before the
// current group's MFMAs and land in registers meanwhile.
// NL: entries of the 36 x ld row image per thread (36 ld / 256, rounded up).
// mask_stride > 0: frames with index 0 (mod mask_stride) contribute nothing (the chain's top level: still being eliminated while this
// runs beside it; k_reduced adds them from their finished images, see DevView::gram_top_stride)
// gather_stride > 0: the chunk is the top level itself -- frames 0, gather_stride, 2 gather_stride, ... (at most 7), summed into the partial
// record behind the dense chunks' (a launch of its own after the top level, where k_reduced does not add these frames itself)
template <int NQ, int NL>
// publish: the record goes out as device-coherent stores and the chunk's ready word follows them (DevView::part_ride: the partial sums ride in the same launch)
__device__ __forceinline__ void chain_gram_chunk(const DevView& v, int chunk, double* R /* 36 x ld */, unsigned short* s_pair /* 128 */, int mask_stride, int gather_stride = 0, bool publish = false) {
  const Ctrl* ct = v.ctrl;
  if (ct->done) return;
  GSTAMP(0);
  const int tid = threadIdx.x, wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63;
  const int D = v.D, ld = v.ldw, N = v.n_frames;
  const int nT = (D + 1 + 15) / 16, nPairs = nT * (nT + 1) / 2;
  const int fstep = gather_stride > 0 ? gather_stride : 1;      // frame slot q of a group is frame (fg + q) fstep
  const int f0 = gather_stride > 0 ? 0 : chunk * v.chunk_frames, f1 = gather_stride > 0 ? (N - 1) / gather_stride + 1 : min(f0 + v.chunk_frames, N);
  double* part = v.part + (size_t)chunk * v.part_stride;
  if (tid < nPairs) {
    int I = 0, J = 0;
    for (int k = 0; k < tid; ++k) if (++J == nT) { ++I; J = I; }
    s_pair[tid] = (unsigned short)(I | (J << 8));
  }
  // this thread's entries of the row image: i = tid + 256 u -> (row, col) by stepping (no division per entry)
  const int step_r = 256 / ld, step_c = 256 - step_r * ld, row0 = tid / ld, col0 = tid - row0 * ld;
  [[maybe_unused]] int gs_ = 1;
  // column-tile pairs are processed in batches of 4 NQ (NQ accumulators per wavefront); more pairs than that re-read the chunk's
  // rows once per batch
  for (int pb = 0; pb < nPairs; pb += 4 * NQ) {
    v4d acc[NQ];
#pragma unroll
    for (int q = 0; q < NQ; ++q) acc[q] = (v4d){0.0, 0.0, 0.0, 0.0};
    double tmp[NL];
    auto request = [&](int fg) {
      const int nrow = min(4, f1 - fg) * 9;
      const double* src = v.cW + (size_t)fg * fstep * 9 * v.ldx;
      const unsigned skip = (unsigned)(fstep - 1) * 9u * (unsigned)v.ldx;      // extra offset per frame slot (0 for consecutive frames)
      unsigned mbits = 0u;                  // bit q: frame fg + q is masked (wave-uniform)
      if (mask_stride > 0) {
#pragma unroll
        for (int q = 0; q < 4; ++q) mbits |= ((fg + q) % mask_stride == 0) ? (1u << q) : 0u;
      }
      int row = row0, col = col0;
#pragma unroll
      for (int u = 0; u < NL; ++u) {
        const unsigned qf = (unsigned)(row * 57) >> 9;               // (row / 9 for rows below 36)
        const bool masked = (mbits >> qf) & 1u;
        tmp[u] = (row < nrow && !masked) ? src[(unsigned)(row * v.ldx + col) + qf * skip] : 0.0;      // (uniform base + 32-bit offset: one register per entry if hoisted)
        row += step_r; col += step_c;
        if (col >= ld) { col -= ld; ++row; }
      }
    };
    request(f0);
    for (int fg = f0; fg < f1; fg += 4) {
#pragma unroll
      for (int u = 0; u < NL; ++u) { const int i = tid + 256 * u; if (i < 36 * ld) R[i] = tmp[u]; }
      __syncthreads();
      GSTAMP(gs_); ++gs_;
      if (fg + 4 < f1) request(fg + 4);
      const double* rq = R + (lane >> 4) * ld + (lane & 15);
      int oa[NQ], ob[NQ];
#pragma unroll
      for (int q = 0; q < NQ; ++q) {
        const int p = min(pb + 4 * q + wave, nPairs - 1);      // (past the end: recomputes the last pair, never written)
        const int ij = s_pair[p];
        oa[q] = (ij & 255) * 16; ob[q] = (ij >> 8) * 16;
      }
#pragma unroll
      for (int ks = 0; ks < 9; ++ks)
#pragma unroll
        for (int q = 0; q < NQ; ++q) acc[q] = __builtin_amdgcn_mfma_f64_16x16x4f64(rq[ks * 4 * ld + oa[q]], rq[ks * 4 * ld + ob[q]], acc[q], 0, 0, 0);
      __syncthreads();
      GSTAMP(gs_); ++gs_;
    }
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
      const int p = pb + 4 * q + wave;
      if (p < nPairs) {
        const int ij = s_pair[p], I = ij & 255, J = ij >> 8;
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          const int row = I * 16 + (lane >> 4) + 4 * g, col = J * 16 + (lane & 15);
          if (row < D && col <= D) {
            double* dst = col < D ? part + row * D + col : part + D * D + row;
            if (publish) __hip_atomic_store(dst, acc[q][g], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); else *dst = acc[q][g];
          }
        }
      }
    }
  }
  if (publish) {
    __builtin_amdgcn_s_waitcnt(0);          // this wavefront's stores have been performed
    __syncthreads();
    if (tid == 0) __hip_atomic_store(v.part_ready + chunk, v.pass_id, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
#ifdef VC_GRAM_STAMPS
  __builtin_amdgcn_s_waitcnt(0);
  GSTAMP(15);
#endif
}
// gather = 0: one workgroup per chunk of consecutive frames (the top level's frames masked out where DevView::gram_top_stride is set);
// gather = 1: one workgroup, the top level's frames into the partial record behind the dense chunks'
template <int NQ, int NL>
__global__ __launch_bounds__(256, 2) void k_chain_gram(DevView v, int gather) {
  extern __shared__ __attribute__((aligned(16))) double R[];    // 36 x ld
  __shared__ unsigned short s_pair[128];                         // pair p -> I | J << 8
  if (gather) chain_gram_chunk<NQ, NL>(v, v.n_chunks, R, s_pair, 0, v.gram_top_stride);
  else chain_gram_chunk<NQ, NL>(v, (int)blockIdx.x, R, s_pair, v.gram_top_stride);
}
// The chain's top level (one group of NW wavefronts side by side, 4-7 dependent eliminations: ~13 us at BASELINE cfg3, 25-50 us with wide
// borders, the chip idle beside it) and, in the same launch, the Gram sums of every frame below it -- final since the launch before:
// workgroup 0 eliminates, workgroups 1 .. n_chunks are k_chain_gram's with the top level's frames masked out (DevView::gram_top_stride).
template <int NW, int NQ, int NL>
__global__ __launch_bounds__(256) void k_chain_top_gram(DevView v, int s, int m, int lvl, int oe) {
  extern __shared__ __attribute__((aligned(16))) double R[];    // 36 x ld
  __shared__ unsigned short s_pair[128];
  __shared__ __attribute__((aligned(16))) double XS[9 * kXsLd];
  __shared__ double An[81];
  __shared__ double Ls_all[NW * 81];
  if (blockIdx.x == 0) {
    // (oe: the top level's frames odd-even on all four wavefronts -- the launcher sized R for it, ChainPlan::oe_top)
    if (NW == 1 && oe) { chain_oe_group(v, s, lvl, 1, 0, R); return; }
    if ((int)threadIdx.x >= 64 * NW) return;      // (a barrier counts the wavefronts that are still there)
    chain_fwd_group<1, NW>(v, s, m, 1, lvl, 0, (int)(threadIdx.x >> 6), XS, An, Ls_all);
    return;
  }
  // (round 6) the workgroup behind the chunks: the camera blocks, the IMU block and the chunk costs of the reduced system, formed here -- beside the
  // top level's dependent eliminations -- instead of inside k_reduced (vc_shared_blocks.hpp; DevView::hadd_early)
  if ((int)blockIdx.x == 1 + v.n_chunks) { hadd_side_job(v, R, 256); return; }
  // ... and behind that one (flag hand-overs, DevView::part_ride): the fixed-order sums of the chunk records, k_part_sum's work without its launch
  if ((int)blockIdx.x > 1 + v.n_chunks) { part_sum_ride_job(v, (int)blockIdx.x - 2 - v.n_chunks, R); return; }
  chain_gram_chunk<NQ, NL>(v, (int)blockIdx.x - 1, R, s_pair, v.gram_top_stride, 0, v.part_ride != 0);
}

// one level of the odd-even elimination (chain_oe_group): a workgroup per group, one wavefront per SIMD; the workgroups behind the groups
// carry the level-1 side job (see k_chain_fwd2)
__global__ __launch_bounds__(256) void k_chain_oe(DevView v, int s, int lvl, int top, int n_groups) {
  __shared__ __attribute__((aligned(16))) double oe_lds[kOeLds];
  // (the side job on the first two wavefronts only, as under k_chain_fwd2<1>: 8 slices per entry, the same fixed order with the switch on and off)
  if ((int)blockIdx.x >= n_groups) { if (threadIdx.x < 128) part_tail_sum_job(v, (int)blockIdx.x - n_groups, oe_lds, 128); return; }
  chain_oe_group(v, s, lvl, top, (int)blockIdx.x, oe_lds);
}

// ------------------------------------------------------------------------------------------ launchers
void launch_imu_delta(const DevView& v, hipStream_t s, int trial) {
  if (v.n_frames < 2) return;
  hipLaunchKernelGGL(k_imu_block, dim3((v.n_frames - 1 + 3) / 4), dim3(256), 0, s, v, trial);      // one wavefront per IMU block
}
void launch_imu_jac(const DevView& v, int wr, hipStream_t s, int trial) {
  if (v.n_frames < 2) return;
  hipLaunchKernelGGL(k_imu_jac, dim3((v.n_frames - 1 + 7) / 8), dim3(256), 0, s, v, wr, trial);      // 8 blocks per workgroup
}
void launch_imu_weights(const DevView& v, int wr, hipStream_t s) {
  if (v.n_frames < 2) return;
  hipLaunchKernelGGL(k_imu_weights, dim3((v.n_frames - 1 + 3) / 4), dim3(64), 0, s, v, wr);      // four blocks per wavefront
}
void launch_chain_gram(const DevView& v, hipStream_t s);
// The levels of the partitioned chain elimination as the plan gives them (vc_chain_plan.hpp).  forward: bottom-up; backward: top-down.
static void chain_levels(const DevView& v, const ChainPlan& p, hipStream_t s, bool forward) {
  const int N = v.n_frames;
  if (N < 1) return;
  const int nl = p.n_levels, top_stride = p.top_stride, m_top = kChainM;      // the top level eliminates whatever is left (fewer than a group)
  const int cpl = (v.D + 1 + 27 + 63) / 64;
  // wide borders: wavefronts side by side (measured in round 2 against several columns per lane: 1.68 -> 1.51 ms per pass at cfg5's per-rank
  // size, 8.74 -> 8.39 ms at its full size; the columns-per-lane instances -- 256 registers + up to 256 accumulation registers, scratch at
  // four columns -- were kept for A/B runs until round 6 and are gone)
  // narrow borders: the levels ChainPlan::two marks are eliminated from both ends (k_chain_fwd2: 4 dependent eliminations per level instead of 7)
  auto fwd = [&](int groups, int stride, int m, int top, int lvl) {
    // (hadd_early: the first launch above the bottom level carries the sums of the chunk records' entries behind S and g_red)
    const int extra = (!top && v.hadd_early && lvl == 1) ? (v.part_stride - (v.D * v.D + v.D) + 15) / 16 : 0;
    if (top ? p.oe_top : p.oe[lvl]) {      // odd-even inside a workgroup of four wavefronts (k_chain_oe: 3 dependent eliminations instead of 4)
      hipLaunchKernelGGL(k_chain_oe, dim3(groups + extra), dim3(256), 0, s, v, stride, lvl, top, groups);
    }
    else if (!top && p.two[lvl]) {
      if (cpl <= 1) hipLaunchKernelGGL(k_chain_fwd2<1>, dim3(groups + extra), dim3(128), 0, s, v, stride, m, lvl, groups);
      else hipLaunchKernelGGL(k_chain_fwd2<2>, dim3(groups + extra), dim3(256), 0, s, v, stride, m, lvl, groups);
    }
    else if (cpl <= 1) hipLaunchKernelGGL((k_chain_fwd<1, 1>), dim3(groups), dim3(64), 0, s, v, stride, m, top, lvl);
    else if (cpl <= 2) hipLaunchKernelGGL((k_chain_fwd<1, 2>), dim3(groups), dim3(128), 0, s, v, stride, m, top, lvl);
    else if (cpl <= 3) hipLaunchKernelGGL((k_chain_fwd<1, 3>), dim3(groups), dim3(192), 0, s, v, stride, m, top, lvl);
    else hipLaunchKernelGGL((k_chain_fwd<1, 4>), dim3(groups), dim3(256), 0, s, v, stride, m, top, lvl);
  };
  if (forward) {
    for (int l = 0; l < nl; ++l) {
      if (l == 0 && v.fold_l0) {      // the chain assembly rides in the bottom level's launch (k_chain_l0)
        if (v.n_cams <= 1) hipLaunchKernelGGL(k_chain_l0<1>, dim3(p.groups[0]), dim3(256), 0, s, v);
        else hipLaunchKernelGGL(k_chain_l0<2>, dim3(p.groups[0]), dim3(256), 0, s, v);
      } else fwd(p.groups[l], p.stride[l], p.m[l], 0, l);
    }
    if (v.gram_top_stride > 0) {
      // early Gram: the top level's one group and the Gram sums of all frames below it in one launch
      const size_t lds_gram = std::max((size_t)36 * v.ldw, (size_t)(v.hadd_early ? kHaddLds : 0)) * sizeof(double);      // (>= 512 doubles: part_sum_ride_job)
      const size_t lds = std::max(lds_gram, (size_t)(p.oe_top ? kOeLds : 0) * sizeof(double));      // (the odd-even top group's images: below the default limit)
      const int ride_blocks = (v.part_ride && v.hadd_early) ? (v.D * v.D + v.D + 15) / 16 : 0;
      const int nT = (v.D + 1 + 15) / 16, nPairs = nT * (nT + 1) / 2, nq = std::min(kMaxPairsPerWaveI, (nPairs + 3) / 4);
      const int nlr = (36 * v.ldw + 255) / 256;
      auto go = [&](auto kern) {
        if (lds_gram > 40000) (void)hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        hipLaunchKernelGGL(kern, dim3(1 + v.n_chunks + (v.hadd_early ? 1 : 0) + ride_blocks), dim3(256), lds, s, v, top_stride, m_top, nl, p.oe_top);
      };
      // (wavefronts of the top group by the border's width, Gram instance by the row image's size: the pairs that occur)
      if (cpl <= 1) { if (nq <= 1) go(k_chain_top_gram<1, 1, 7>); else go(k_chain_top_gram<1, 2, 7>); }
      else if (cpl <= 2) { if (nlr <= 12) go(k_chain_top_gram<2, 4, 12>); else if (nq <= 6) go(k_chain_top_gram<2, 6, 16>); else go(k_chain_top_gram<2, 9, 16>); }
      else if (cpl <= 3) { if (nlr <= 16) go(k_chain_top_gram<3, 9, 16>); else if (nlr <= 21) go(k_chain_top_gram<3, 9, 21>); else go(k_chain_top_gram<3, 9, 25>); }
      else { if (nlr <= 25) go(k_chain_top_gram<4, 9, 25>); else go(k_chain_top_gram<4, 9, 30>); }
    } else {
      fwd(1, top_stride, m_top, 1, nl);
    }
  } else {
    // the whole back-substitution as one launch without hand-overs (k_chain_back_path): any border width, sharded passes included
    if (v.back_path && nl >= 1 && nl <= 5) {
      BackPath P; P.n = nl;
      for (int l = 0; l < 6; ++l) { P.stride[l] = l < nl ? p.stride[l] : 1; P.m[l] = l < nl ? p.m[l] : 2; P.two[l] = l < nl ? (p.oe[l] ? 2 : p.two[l]) : 0; }
      const bool ct0 = v.D + 1 > kPathRowCols;
      P.oe_top = p.oe_top; P.top_stride = top_stride; P.ldr = ct0 ? 1 : ((v.D + 1) | 1); P.dsw = ((v.D + 63) / 64) * 64;
      if (ct0) hipLaunchKernelGGL(k_chain_t0, dim3((N + 3) / 4), dim3(256), 0, s, v);
      const int nw = nl + 1;
      P.tail = (v.tail_deferred && nw >= 4) ? 1 : 0;
      const size_t lds = std::max(((size_t)nw * kPathDl + (size_t)nw * P.dsw + 4 + (ct0 ? 0 : (size_t)nw * 63 * P.ldr)), (size_t)(P.tail ? kTailLds : 0)) * sizeof(double);
      static LdsGrant g4, g6;
      auto go = [&](auto kern, LdsGrant& g) {
        if (lds > 60000 && g.need(lds)) (void)hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        hipLaunchKernelGGL(kern, dim3(p.groups[0] + P.tail), dim3(64 * nw), lds, s, v, P);
      };
      if (nw <= 4) { if (ct0) go(k_chain_back_path<4, true>, g4); else go(k_chain_back_path<4, false>, g4); }
      else { if (ct0) go(k_chain_back_path<6, true>, g6); else go(k_chain_back_path<6, false>, g6); }
      return;
    }
    hipLaunchKernelGGL(k_chain_back, dim3(1 + (nl > 0 ? (N + kBackT0Frames - 1) / kBackT0Frames : 0)), dim3(64), 0, s, v, top_stride, m_top, 1, nl, p.oe_top ? 2 : 0);
    // the levels below: one launch (k_chain_back_levels: ready words instead of kernel boundaries)
    // (only while every workgroup of the launch can be resident at once -- 119 registers, 4 wavefronts per SIMD, 4096 on the chip; half of
    //  that here: a group that waits for its separators then never keeps a producer from starting, whatever order the dispatcher picks)
    int total_groups = 0;
    for (int l = 0; l < nl; ++l) total_groups += p.groups[l];
    // (half of what the device can hold of this kernel -- asked once, not a constant of one chip: the other half is left to whatever the
    //  second stream runs beside it)
    static const int resident_limit = [] {
      int dev = 0, per_cu = 0; hipDeviceProp_t pr;
      if (hipGetDevice(&dev) != hipSuccess || hipGetDeviceProperties(&pr, dev) != hipSuccess ||
          hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, (const void*)k_chain_back_levels, 64, 0) != hipSuccess || per_cu <= 0) return 2048;
      return std::max(64, per_cu * pr.multiProcessorCount / 2);
    }();
    if (nl > 0 && nl <= 8 && v.cready && total_groups <= resident_limit) {
      BackLevels L; L.n = nl;
      int at = 0;
      for (int i = 0; i < nl; ++i) {
        const int l = nl - 1 - i;
        L.start[i] = at; L.stride[i] = p.stride[l]; L.m[i] = p.m[l]; L.two[i] = p.oe[l] ? 2 : p.two[l];
        at += p.groups[l];
      }
      for (int i = nl; i < 8; ++i) { L.start[i] = 1 << 30; L.stride[i] = 1; L.m[i] = 2; L.two[i] = 0; }
      hipLaunchKernelGGL(k_chain_back_levels, dim3(at), dim3(64), 0, s, v, L);
    } else
    for (int l = nl - 1; l >= 0; --l)
      hipLaunchKernelGGL(k_chain_back, dim3(p.groups[l]), dim3(64), 0, s, v, p.stride[l], p.m[l], 0, l, p.oe[l] ? 2 : p.two[l]);
  }
}
void launch_chain_init(const DevView& v, hipStream_t s) {
  const size_t slot = (size_t)v.n_cams * kGStride + kGStride;
  const size_t lds = std::max((size_t)4 * (v.n_cams * kGStride + kInitPad), 4 * slot) * sizeof(double);
  auto go = [&](auto kern) {
    if (lds > 65536) (void)hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    hipLaunchKernelGGL(kern, dim3(v.n_chunks), dim3(256), lds, s, v);
  };
  if (v.n_cams <= 1) go(k_chain_init<1>); else if (v.n_cams <= 2) go(k_chain_init<2>); else if (v.n_cams <= 4) go(k_chain_init<4>); else go(k_chain_init<8>);
}
void launch_chain_fwd(const DevView& v, const ChainPlan& p, hipStream_t s) { chain_levels(v, p, s, true); }
static void chain_gram_go(const DevView& v, hipStream_t s, int gather) {
  const size_t lds = (size_t)36 * v.ldw * sizeof(double);
  const int nT = (v.D + 1 + 15) / 16, nPairs = nT * (nT + 1) / 2, nq = std::min(kMaxPairsPerWaveI, (nPairs + 3) / 4);
  auto go = [&](auto kern) {
    if (lds > 65536) (void)hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    hipLaunchKernelGGL(kern, dim3(gather ? 1 : v.n_chunks), dim3(256), lds, s, v, gather);
  };
  // (pairs per wavefront, row-image entries per thread) by the number of column tiles: ld = 48, 80, 112, 144, 176, 208
  const int nl = (36 * v.ldw + 255) / 256;
  if (nl <= 7) { if (nq <= 1) go(k_chain_gram<1, 7>); else go(k_chain_gram<2, 7>); }
  else if (nl <= 12) go(k_chain_gram<4, 12>);
  else if (nl <= 16) { if (nq <= 6) go(k_chain_gram<6, 16>); else go(k_chain_gram<9, 16>); }
  else if (nl <= 21) go(k_chain_gram<9, 21>);
  else if (nl <= 25) go(k_chain_gram<9, 25>);
  else go(k_chain_gram<9, 30>);
}
void launch_chain_gram(const DevView& v, hipStream_t s) { chain_gram_go(v, s, 0); }
// early Gram where k_reduced does not add the top level's frames itself (D > kEarlyTopD, sharded passes): their sums as one more partial record
void launch_chain_gram_top(const DevView& v, hipStream_t s) { chain_gram_go(v, s, 1); }
void launch_chain_solve_b(const DevView& v, const ChainPlan& p, hipStream_t s) { chain_levels(v, p, s, false); }

}  // namespace vc
