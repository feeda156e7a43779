// vci_chain_init.hpp -- k_chain_init: wavefront per frame: 9 x 9 diagonal block (visual tiles + two IMU blocks), coupling to the next frame,
// dense border row W (9 x D) and gradient; damping; per-chunk sums of the camera Gram blocks and of the IMU shared-parameter block.
// Kernel fragment of vc_imu_kernels.hip alone (defines __global__ symbols; included there in stage order; not for host harnesses).
#pragma once
#include <hip/hip_runtime.h>
#include "vc_math.hpp"
#include "vc_device.h"
#include "vc_kutil.hpp"

namespace vc {

// ------------------------------------------------------------------------------------------ chain assembly
// One wavefront per frame, one workgroup per chunk (groups of 4 frames).  The frame's image is written ONCE, column by column
// (lane = image column: border [W | g], then the blocks [C | A | B]): every column gathers what belongs in it -- the camera's
// columns from the frame's tile of that camera, the IMU-parameter columns and the 9 x 9 blocks from the two IMU blocks the frame
// takes part in (compact records, vc_device.h: kSeg*), the right-hand side, the separator couplings of a sharded chain -- instead
// of zero-filling the image and scattering into it (round 2: 22 of 45 MB per launch at BASELINE cfg3 were the zero-fill and the
// unread parts of the 33 x 33 blocks).  The padding columns between D + 1 and ldw and behind the blocks are never read.
#ifdef VC_INIT_STAMPS
#define ISTAMP(i) do { if (blockIdx.x == gridDim.x / 2 && threadIdx.x == 0 && (i) < 16) v.dbg[i] = (long long)__builtin_amdgcn_s_memrealtime(); } while (0)
#else
#define ISTAMP(i) do { } while (0)
#endif
constexpr int kInitPad = 160;            // per wavefront behind the Gram records: Hs 42 | A 81 | g 9 | lambda 9 | tile cameras 8 | pad
// Round 5: the loads of a frame are two dependent round trips instead of four (the frame's tile of every camera comes from
// frame_cam_tile[f][c] -- requested before the control record has arrived; then everything else in one go: the tiles' Gram records, the
// two IMU records, costs, damping state -- where round 4 walked frame_tile_off -> tile_cam -> IMU records -> Gram records), and a
// wavefront that owns several frames of its chunk (large problems: the chunk grows with the frame count so that the whole grid is
// resident at once) requests frame i + 1's data before it forms frame i's columns: a frame costs its arithmetic, not arithmetic + latency.
// Stamps (tools/init_stamps.py) before the change: ~10 us of the ~20 us a frame took at every size were the four round trips.
// CMAX: cameras the instance holds registers for (1, 2, 4, 8).
template <int CMAX>
struct InitLoads {
  double gv[CMAX][3];          // Gram record of the frame's tile of camera c as it lies in HBM (packed upper triangle + side vector: entries lane, lane + 64, lane + 128 of kGPack)
  double pre[9];               // lanes 0..14: couplings of IMU parameter `lane`; lanes 15..23: column lane - 15 of B
  double a_imu[2], g_imu, sc2_in, dg_in, isum_in[4], cost_in;
};
template <int CMAX>
__global__ __launch_bounds__(256, 2) void k_chain_init(DevView v) {     // (two workgroups per CU: the kernel waits on memory)
  // Chunk sums of the camera Gram blocks and of the IMU shared block: per-lane accumulators across the frame loop (instances up to four
  // cameras) or a pass of their own behind it (eight cameras, round 6: CMAX x 3 + 4 accumulators beside CMAX x 3 + 4 doubles of the frame in
  // flight kept 76 registers in scratch there -- 304 B per lane --, and a scratch reload waits for every load requested before it, the next
  // frame's among them: k_chain_init 107 -> 91 us at 6250 frames x 8 cameras; with four cameras the second read of the records costs more than
  // the 84 B of scratch did: 35 -> 37 us at 2500 frames)
  constexpr bool kLoopSums = CMAX <= 4;
  constexpr int CS = kLoopSums ? CMAX : 1;
  extern __shared__ __attribute__((aligned(16))) double sh[];
  __shared__ CamDesc s_cd[kMaxCams];
  __shared__ double s_R[kMaxCams * 9];   // the cameras' rotations R_ck, once per workgroup
  __shared__ int s_ci[256];              // what every image column is: owning camera (255: none) | column inside its block << 8 | "comes from the IMU records" << 16
  const Ctrl* ct = v.ctrl;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int C = v.n_cams, D = v.D, N = v.n_frames, ldw = v.ldw, ldx = v.ldx, nW = D + 1, ncol = nW + 27;
  const int chunk = blockIdx.x;
  const int f0 = chunk * v.chunk_frames, f1 = min(f0 + v.chunk_frames, N);
  // the first frame's tile list does not depend on the control record: requested ahead of it
  auto load_fct = [&](int f) { return (lane < C && f < f1) ? v.frame_cam_tile[(size_t)f * C + lane] : -1; };
  int fct = load_fct(f0 + wave);
#ifdef VC_INIT_STAMPS
  const long long ist0_ = (long long)__builtin_amdgcn_s_memrealtime();
#endif
  if (ct->done) return;
#ifdef VC_INIT_STAMPS
  if (blockIdx.x == gridDim.x / 2 && threadIdx.x == 0) v.dbg[0] = ist0_;      // (not in passes that exit early)
#endif
  const int cur = ct->cur;
  const int init_scale = ct->init_scale, reuse = ct->reuse_diag;
  const double radius = ct->radius;
  int sp_col = -1;                                 // lanes 0..14: the column of IMU parameter `lane` (or none)
#pragma unroll
  for (int a = 0; a < 15; ++a) sp_col = (lane == a) ? v.imu_param_col[a] : sp_col;
  // ---- everything a frame needs from memory, requested in one go (fct_f: lane c's tile of camera c in frame f, or -1)
  auto issue = [&](int f, int fct_f, InitLoads<CMAX>& R) {
    const bool live = f < f1;
    const bool pin_f = (f == 0 && v.pin_first), pin_l = (f == N - 1 && v.pin_last), pin_self = pin_f || pin_l;
    const bool pin_next = (f + 1 == N - 1 && v.pin_last);
    const double* rc = (live && f >= 1) ? v.segb[cur] + (size_t)(f - 1) * kSegStride : nullptr;
    const double* rp = (live && f + 1 < N) ? v.segb[cur] + (size_t)f * kSegStride : nullptr;
#pragma unroll
    for (int c = 0; c < CMAX; ++c) {
      const int tc = __builtin_amdgcn_readfirstlane(__shfl(fct_f, c, 64));      // (wave-uniform: a scalar branch per camera)
#pragma unroll
      for (int q = 0; q < 3; ++q) R.gv[c][q] = 0.0;
      if (c < C && tc >= 0) {
        const double* g = v.Gb[cur] + (size_t)tc * kGPack;      // (three contiguous loads per tile; expanded to the 16 x 16 form on the way into LDS)
#pragma unroll
        for (int q = 0; q < 3; ++q) { const int e = q * 64 + lane; const double x = g[e < kGPack ? e : 0]; R.gv[c][q] = e < kGPack ? x : 0.0; }
      }
    }
    // Branch-free from here on: every lane loads from a valid address (a lane without an entry reads the start of record 0) and keeps
    // the value or a zero by a select.  Loads under divergent branches are not hoisted out of them: round 4's form -- `if (lane has this
    // entry) x += record[..]`, ~40 masked loads per frame -- ran them as a chain of dependent round trips, 8 of the 17 us a wavefront
    // took at BASELINE cfg3 and 60 of 124 us at cfg5's per-rank size (tools/init_stamps.py on a build of the kernel without the IMU-record loads).
    const double* safe = v.cg;                 // (always there; only its first entry is ever read through `safe`, and the value is dropped)
    const double* rcs = rc ? rc : safe;
    const double* rps = rp ? rp : safe;
    const bool has_c = rc != nullptr, has_p = rp != nullptr;      // wave-uniform
    const int oc = has_c ? 1 : 0, op = has_p ? 1 : 0;             // offsets into an absent record collapse to 0
    {
      const bool tile_cost = lane < C && fct_f >= 0, blk_cost = lane == 8 && has_c;      // every block counted once, by its "cur" frame
      const double* pcst = tile_cost ? v.tile_costb[cur] + fct_f : (blk_cost ? v.seg_costb[cur] + (f - 1) : safe);      // (has_c: f >= 1 and a block f - 1 exists)
      const double x = *pcst;
      R.cost_in = (tile_cost || blk_cost) ? x : 0.0;
    }
    {
      // lanes 0..14: IMU parameter `lane`'s couplings with this frame (from both records); lanes 15..23: column lane - 15 of B
      const bool isB = lane >= 15 && lane < 24 && has_p && !pin_self && !pin_next;
      const bool par = lane < 15 && sp_col >= 0;
      const int a = lane < 15 ? lane : 0, jb = lane >= 15 && lane < 24 ? lane - 15 : 0;
      const double* pa = par ? rcs + (kSegWc + a) * oc : (isB ? rps + kSegBpc + jb : safe);
      const int sa = par ? 15 * oc : (isB ? 9 : 0);
      const bool va = (par && has_c) || isB;
      const double* pb = par ? rps + (kSegWp + a) * op : safe;
      const int sb = par ? 15 * op : 0;
      const bool vb = par && has_p;
      double xa[9], xb[9];
#pragma unroll
      for (int i = 0; i < 9; ++i) { xa[i] = pa[i * sa]; xb[i] = pb[i * sb]; }
#pragma unroll
      for (int i = 0; i < 9; ++i) R.pre[i] = (va ? xa[i] : 0.0) + (vb ? xb[i] : 0.0);
    }
    {
      double xc[2], xp[2];
#pragma unroll
      for (int q = 0; q < 2; ++q) { const int e = lane + 64 * q, ee = e < 81 ? e : 0; xc[q] = rcs[(kSegAcc + ee) * oc]; xp[q] = rps[(kSegApp + ee) * op]; }
#pragma unroll
      for (int q = 0; q < 2; ++q) { const bool in = lane + 64 * q < 81; R.a_imu[q] = ((in && has_c) ? xc[q] : 0.0) + ((in && has_p) ? xp[q] : 0.0); }
    }
    {
      const int l9 = lane < 9 ? lane : 0;
      const size_t fo = (size_t)(live ? f : 0) * 9 + l9;
      const double gc = rcs[(kSegGc + l9) * oc], gp = rps[(kSegGp + l9) * op], s2 = v.cscale2[fo], dgv = v.cdiag[fo];
      const bool in = lane < 9 && live;
      R.g_imu = ((in && has_c) ? gc : 0.0) + ((in && has_p) ? gp : 0.0);
      R.sc2_in = (in && !init_scale) ? s2 : 0.0;
      R.dg_in = (in && reuse) ? dgv : 0.0;
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) {      // IMU shared block of block f-1 (every block counted once, by its "cur" frame)
      const int e = lane + 64 * q, a = e >> 4, b2 = e & 15;
      const bool in = a < 15;
      if (kLoopSums) {
        const double x = rcs[(in ? ((b2 < 15) ? kSegHii + a * 15 + b2 : kSegGi + a) : 0) * oc];
        R.isum_in[q] = (in && has_c) ? x : 0.0;
      } else R.isum_in[q] = 0.0;
    }
  };
  InitLoads<CMAX> R;
  issue(f0 + wave, fct, R);
  int fct_next = load_fct(f0 + wave + 4);          // the tile list of the frame after this one (one load, a frame ahead of its use)
  if (tid < kMaxCams) s_cd[tid] = v.cd[tid];
  if (tid < C) { double Rm[9]; quat_to_R(v.cams[cur] + (size_t)tid * kCamStride, Rm); for (int k = 0; k < 9; ++k) s_R[tid * 9 + k] = Rm[k]; }
  double* Gw = sh + wave * (C * kGStride + kInitPad);
  double* Hs = Gw + C * kGStride;
  double* As = Hs + 42;                  // the frame's own 9 x 9 block (undamped)
  double* gs = As + 81;                  // its right-hand side
  double* ls = gs + 9;                   // its damping
  int* tcam = reinterpret_cast<int*>(ls + 9);      // cameras of the frame's tiles [8], then the frame's tile of every camera [8]
  int* tinv = tcam + kMaxCams;
  double gsum[CS][3];           // per-camera sums of the chunk's Gram records, packed like the records (kLoopSums)
  // where the lane's packed entries go in the 16 x 16 + 16 record: offset of (r, c), of (c, r), -1: no such entry
  int po[3], pm[3];
#pragma unroll
  for (int q = 0; q < 3; ++q) {
    const int e = q * 64 + lane;
    int r = 0;
#pragma unroll
    for (int a = 1; a < 16; ++a) r += (e >= a * 16 - (a * (a - 1)) / 2) ? 1 : 0;      // row of packed entry e (< kGPackGrad)
    const int cidx = r + (e - (r * 16 - (r * (r - 1)) / 2));
    po[q] = e < kGPackGrad ? r * 16 + cidx : (e < kGPack ? kGGrad + (e - kGPackGrad) : -1);
    pm[q] = (e < kGPackGrad && cidx != r) ? cidx * 16 + r : -1;
  }
  double isum[4] = {0.0, 0.0, 0.0, 0.0};      // IMU shared block: Hii[a][b] at a*16+b (a,b<15), g_i[a] at a*16+15
  double csum = 0.0;            // cost at the linearisation point: the frames' tiles (lanes 0..7) and IMU blocks (lane 8), summed per chunk here
                                // instead of over all tiles and blocks by the one workgroup of k_reduced (32 of its 214 us at 50 000 tiles)
#pragma unroll
  for (int c = 0; c < CS; ++c)
#pragma unroll
    for (int q = 0; q < 3; ++q) gsum[c][q] = 0.0;
  // what each image column is, once for all frames of the chunk: owning camera and column inside its block; the columns that come
  // from the IMU records -- the (at most 15) IMU-parameter columns and the 9 columns of B -- belong to lanes 0..23 whatever their
  // position in the image, so that their values can be requested before anything else happens
  if (tid < ncol) {
    const int col = tid, e = col - nW;
    int cam = 255, loc = 0, skip = (e >= 18 && e < 27) ? 1 : 0;
    if (col < D) {
      const int cc = v.col_cam[col];
      cam = cc >= 0 ? cc : 255; loc = v.col_local[col];
#pragma unroll
      for (int a = 0; a < 15; ++a) skip |= (v.imu_param_col[a] == col) ? 1 : 0;
    }
    s_ci[col] = cam | (loc << 8) | (skip << 16);
  }
  __syncthreads();
  ISTAMP(1);

  for (int fg = f0; fg < f1; fg += 4) {
    const int f = fg + wave;
    if (f >= f1) continue;
    double* Wf = v.cW + (size_t)f * 9 * ldx;     // the frame's image: [W | g] in columns 0..D, then (from ldw) C (zero) | A | B
    // pinned frames (separator / ghost, see DevView): their rows go to sep_strip, the chain sees an isolated identity block
    const bool pin_f = (f == 0 && v.pin_first), pin_l = (f == N - 1 && v.pin_last), pin_self = pin_f || pin_l;
    const bool pin_prev = (f == 1 && v.pin_first), pin_next = (f + 1 == N - 1 && v.pin_last);
    double* Wt = pin_self ? v.sep_strip + (size_t)(pin_f ? 0 : 1) * 9 * ldw : Wf;
    const int ldt = pin_self ? ldw : ldx;         // row stride of Wt
    const int sep_self = pin_f ? v.sep_col0 : v.sep_col1;
    const double* rc = (f >= 1) ? v.segb[cur] + (size_t)(f - 1) * kSegStride : nullptr;      // (the separator couplings below read them again: L2 hits)
    const double* rp = (f + 1 < N) ? v.segb[cur] + (size_t)f * kSegStride : nullptr;
    // ---- this frame's values out of the load registers: Gram records to LDS and into the chunk's per-camera sums, the rest to locals
    const unsigned long long present = __ballot(lane < C && fct >= 0);
    const int nt = __popcll(present);
    if (lane < kMaxCams) {
      const bool have = lane < C && fct >= 0;
      const int slot = __popcll(present & ((1ull << lane) - 1ull));
      tinv[lane] = have ? slot : -1;                       // the frame's tile slot of every camera
    }
    wave_lds_sync_local();      // (wavefront scope: a workgroup-scope fence would wait for the next frame's loads)
    if (lane < C && fct >= 0) tcam[tinv[lane]] = lane;     // camera of every slot
    csum += R.cost_in;
    if (kLoopSums) {
#pragma unroll
      for (int q = 0; q < 4; ++q) isum[q] += R.isum_in[q];
    }
    int slot_c = 0;
#pragma unroll
    for (int c = 0; c < CMAX; ++c) {
      const bool have = c < C && ((present >> c) & 1ull);      // wave-uniform
      if (have) {
#pragma unroll
        for (int q = 0; q < 3; ++q) {
          if (po[q] >= 0) Gw[slot_c * kGStride + po[q]] = R.gv[c][q];
          if (pm[q] >= 0) Gw[slot_c * kGStride + pm[q]] = R.gv[c][q];
          if (kLoopSums) gsum[c < CS ? c : 0][q] += R.gv[c][q];
        }
        ++slot_c;
      }
    }
    // the image columns that come straight from the IMU records (lanes 0..23) are written now: their registers are free for the next
    // frame's loads
    if (sp_col >= 0) {
#pragma unroll
      for (int i = 0; i < 9; ++i) Wt[i * ldt + sp_col] = R.pre[i];
      if (pin_self) {
#pragma unroll
        for (int i = 0; i < 9; ++i) Wf[i * ldx + sp_col] = 0.0;
      }
    }
    if (lane >= 15 && lane < 24) {
#pragma unroll
      for (int i = 0; i < 9; ++i) Wf[i * ldx + ldw + 18 + (lane - 15)] = R.pre[i];
    }
    const double a_imu[2] = {R.a_imu[0], R.a_imu[1]};
    const double g_imu = R.g_imu, sc2_in = R.sc2_in, dg_in = R.dg_in;
    wave_lds_sync_local();
    ISTAMP(2);
    // ---- the next frame of this wavefront: its loads go out now, under this frame's arithmetic and stores
    fct = fct_next;
    if (f + 4 < f1) { issue(f + 4, fct, R); fct_next = load_fct(f + 8); }
    ISTAMP(3);
    // ---- visual part of the frame's own block: H_pp (6 x 6) and g_p (6) from the tiles (lanes 0..41)
    if (lane < 42) {
      double hval = 0.0;
      for (int t = 0; t < nt; ++t) {
        const int c = tcam[t];
        const double* Rm = s_R + c * 9;
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
    wave_lds_sync_local();
    ISTAMP(4);
    // ---- own block A (lane e = 9 i + j, two slots), right-hand side, damping
    double aval[2];
#pragma unroll
    for (int q = 0; q < 2; ++q) {
      const int e = lane + 64 * q, i = e / 9, j = e % 9;
      aval[q] = a_imu[q] + ((e < 81 && i < 6 && j < 6) ? Hs[i * 6 + j] : 0.0);
      if (e < 81) As[e] = aval[q];
    }
    const double gval = g_imu + ((lane < 6) ? Hs[36 + lane] : 0.0);
    double hd = 0.0;
    // diagonal entry i lives in lane (i*10) % 64, slot (i*10) / 64
#pragma unroll
    for (int i = 0; i < 9; ++i) {
      const int e = i * 10;
      const double d = readlane_f64(aval[e >> 6], e & 63);
      if (lane == i) hd = d;
    }
    if (lane < 9) {
      // damping of the 9 frame parameters (Jacobi scaling fixed per Solve, diagonal re-used after rejections)
      double sc2 = sc2_in, dg = dg_in;
      if (init_scale) { sc2 = jacobi_scale2(hd); v.cscale2[(size_t)f * 9 + lane] = sc2; }
      if (!reuse) { dg = lm_clamped_diag(hd, sc2); v.cdiag[(size_t)f * 9 + lane] = dg; }
      const double lam = pin_self ? 0.0 : dg / (radius * sc2);
      v.clam[(size_t)f * 9 + lane] = lam;
      v.cg[(size_t)f * 9 + lane] = pin_self ? 0.0 : gval;
      gs[lane] = gval; ls[lane] = lam;
    }
    wave_lds_sync_local();
    ISTAMP(5);
    // ---- the image: every column written once (the columns that come from the IMU records went out above); one column per lane and round
    for (int col = lane; col < ncol; col += 64) {
      const int ci = s_ci[col];
      if (ci >> 16) continue;
      double val[9];
#pragma unroll
      for (int i = 0; i < 9; ++i) val[i] = 0.0;
      const int e = col - nW, jb = (e >= 0) ? e % 9 : 0;
      const int cc = ci & 255, j = (ci >> 8) & 255;
      const int t = (cc < kMaxCams) ? tinv[cc] : -1;
      if (col < D && t >= 0) {                     // a camera's column: from the frame's tile of that camera
        const int flags = s_cd[cc].flags, nrot = (flags & kCamRotFree) ? 3 : 0, ntr = (flags & kCamTransFree) ? 3 : 0;
        const double* Rm = s_R + cc * 9;
        const double* g = Gw + t * kGStride;
        double u[6];
        if (j < nrot) {
#pragma unroll
          for (int r = 0; r < 6; ++r) u[r] = -(g[r * 16 + 3] * Rm[j] + g[r * 16 + 4] * Rm[3 + j] + g[r * 16 + 5] * Rm[6 + j]);
        } else {
          const int jj = (j < nrot + ntr) ? j - nrot : 6 + (j - nrot - ntr);
#pragma unroll
          for (int r = 0; r < 6; ++r) u[r] = g[r * 16 + jj];
        }
#pragma unroll
        for (int i = 0; i < 3; ++i) {
          val[i] = -(Rm[i] * u[0] + Rm[3 + i] * u[1] + Rm[6 + i] * u[2]);
          val[3 + i] = Rm[i] * u[3] + Rm[3 + i] * u[4] + Rm[6 + i] * u[5];
        }
      }
      // a separator's columns (sharded chain): the coupling of this frame with the pinned neighbour, from the shared IMU block
      if (col < D && pin_prev && rc && col >= v.sep_col0 && col < v.sep_col0 + 9) {       // rows: this frame (cur), cols: the pinned frame 0 (prev)
#pragma unroll
        for (int i = 0; i < 9; ++i) val[i] = rc[kSegBpc + (col - v.sep_col0) * 9 + i];
      }
      if (col < D && pin_next && rp && col >= v.sep_col1 && col < v.sep_col1 + 9) {       // rows: this frame (prev), cols: the pinned last frame (cur)
#pragma unroll
        for (int i = 0; i < 9; ++i) val[i] = rp[kSegBpc + i * 9 + (col - v.sep_col1)];
      }
      if (col < D && pin_self && col >= sep_self && col < sep_self + 9) {                 // a pinned frame's own block sits in its separator columns
#pragma unroll
        for (int i = 0; i < 9; ++i) val[i] += As[i * 9 + (col - sep_self)];
      }
      if (col == D) {                              // the right-hand side rides as column D
#pragma unroll
        for (int i = 0; i < 9; ++i) val[i] = gs[i];
      }
      if (e >= 9 && e < 18) {                      // A (damped; a pinned frame: the identity)
#pragma unroll
        for (int i = 0; i < 9; ++i) val[i] = pin_self ? ((i == jb) ? 1.0 : 0.0) : As[i * 9 + jb] + ((i == jb) ? ls[i] : 0.0);
      }
      if (col < nW) {
#pragma unroll
        for (int i = 0; i < 9; ++i) Wt[i * ldt + col] = val[i];
        if (pin_self) {                            // (wave-uniform) the chain's image of a pinned frame has an empty border
#pragma unroll
          for (int i = 0; i < 9; ++i) Wf[i * ldx + col] = 0.0;
        }
      } else {
#pragma unroll
        for (int i = 0; i < 9; ++i) Wf[i * ldx + ldw + e] = val[i];
      }
    }
    wave_lds_sync_local();
    ISTAMP(6);
  }
  __syncthreads();
  ISTAMP(7);
  double* part = v.part + (size_t)chunk * v.part_stride;
  if constexpr (kLoopSums) {
    // (4 wavefronts combined in fixed order)
    const int slot = C * kGStride + kGStride;
#pragma unroll
    for (int c = 0; c < CS; ++c)
      if (c < C) {
#pragma unroll
        for (int q = 0; q < 3; ++q) {
          if (po[q] >= 0) sh[wave * slot + c * kGStride + po[q]] = gsum[c][q];
          if (pm[q] >= 0) sh[wave * slot + c * kGStride + pm[q]] = gsum[c][q];
        }
      }
#pragma unroll
    for (int q = 0; q < 4; ++q) sh[wave * slot + C * kGStride + q * 64 + lane] = isum[q];
    __syncthreads();
    for (int e = tid; e < slot; e += 256)
      part[D * D + D + e] = (sh[e] + sh[slot + e]) + (sh[2 * slot + e] + sh[3 * slot + e]);
  } else {
    // second reads of the chunk's records (out of the L2 / the memory-side cache), frame by frame in fixed order
    int* tl = reinterpret_cast<int*>(sh);                 // the chunk's tile table [frame][camera] (the frame loop is done with the LDS)
    const int nf = f1 - f0;
    for (int e = tid; e < nf * C; e += 256) tl[e] = v.frame_cam_tile[(size_t)f0 * C + e];
    __syncthreads();
    const double* Gc = v.Gb[cur];
    for (int e = tid; e < C * kGPack; e += 256) {
      const int c = e / kGPack, pe = e - c * kGPack;
      double acc = 0.0;
      for (int fr = 0; fr < nf; fr += 8) {               // eight frames' loads in flight, added in frame order
        double x[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) { const int t = fr + u < nf ? tl[(fr + u) * C + c] : -1; const double y = Gc[t >= 0 ? (size_t)t * kGPack + pe : 0]; x[u] = t >= 0 ? y : 0.0; }
#pragma unroll
        for (int u = 0; u < 8; ++u) acc += x[u];
      }
      // where the packed entry goes in the 16 x 16 + 16 record: (r, c) and (c, r), or the side vector
      int r = 0;
#pragma unroll
      for (int a2 = 1; a2 < 16; ++a2) r += (pe >= a2 * 16 - (a2 * (a2 - 1)) / 2) ? 1 : 0;
      const int cidx = r + (pe - (r * 16 - (r * (r - 1)) / 2));
      double* pc = part + D * D + D + c * kGStride;
      if (pe < kGPackGrad) { pc[r * 16 + cidx] = acc; if (cidx != r) pc[cidx * 16 + r] = acc; }
      else pc[kGGrad + (pe - kGPackGrad)] = acc;
    }
    {   // IMU shared block of the blocks f - 1, f in the chunk: Hii[a][b] at a*16+b (a, b < 15), g_i[a] at a*16+15
      const int e = tid, a2 = e >> 4, b2 = e & 15;
      const bool in = a2 < 15;
      const int off = in ? ((b2 < 15) ? kSegHii + a2 * 15 + b2 : kSegGi + a2) : 0;
      double acc = 0.0;
      for (int fr = 0; fr < nf; fr += 8) {
        double x[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) { const int f = f0 + fr + u; const bool has = in && fr + u < nf && f >= 1; const double y = v.segb[cur][has ? (size_t)(f - 1) * kSegStride + off : 0]; x[u] = has ? y : 0.0; }
#pragma unroll
        for (int u = 0; u < 8; ++u) acc += x[u];
      }
      part[D * D + D + C * kGStride + e] = acc;
    }
  }
  // the chunk's cost: nine lanes per wavefront hold terms; fixed order (lane, then wavefront)
  __syncthreads();
  if (lane < 9) sh[wave * 9 + lane] = csum;
  __syncthreads();
  if (tid == 0) {
    double t = 0.0;
    for (int w = 0; w < 4; ++w) { double tw = 0.0; for (int k = 0; k < 9; ++k) tw += sh[w * 9 + k]; t += tw; }
    part[v.part_stride - 1] = t;
  }
#ifdef VC_INIT_STAMPS
  __builtin_amdgcn_s_waitcnt(0);
  ISTAMP(8);
#endif
}

}  // namespace vc
