// vc_target_refine.hip -- one Gauss-Newton step on the calibration target's points, the frame poses and the shared camera columns marginalised,
// on the GPU (gfx950, wave64, fp64): vc_target_refine_batch.  vc_target_refine.hpp has the arithmetic and the definition.
//
//   k_tr_sweep     one wavefront per frame, two per workgroup, no workgroup barrier (modelled on k_select_info).  Lanes stride over the corners
//                  of each view: the Gram block and its gradient by wave_allsum, the corner's own record (J_f^T J_p, J_p^T J_p, J_p^T r,
//                  J_p^T J_s) stored per corner.  After the last view the 6 x 6 Cholesky (every lane), L^-1 W and L^-1 g_f with lane = column,
//                  the frame's share of S_ss / g_s, and the lanes stride over the frame's (frame, point) records: the corners of one point
//                  summed in camera order, y = L^-1 sum F solved and stored.
//   k_tr_assemble  grid (point, column chunk): thread = one 3 x 3 block (p, p') of S_dd in registers, the frames of p walked in ascending order
//                  through the by-point list; the last chunk holds the columns of s, the gradient and the point's corner count.  One writer per
//                  entry, no atomic.
//   k_tr_shared    one workgroup: S_ss and g_s summed in frame order, scaled, + 1e-6 I, factored with lane = column (sel_chol_step).
//   k_tr_zrows     thread = row of S_ds: z = U^-T (c o row), times sqrt(pivot).      k_tr_rank: S_dd -= Z Z^T, g_d -= Z z_g (the rank-D update).
//   k_tr_gauge     one workgroup: observed points, centroid, Q by modified Gram-Schmidt (fixed-order sums), Pi (points - nominal), Pi b, mu.
//   k_tr_mq        V = M Q.      k_tr_gauge2: Q^T V, R = V - Q (Q^T V + mu I) / 2, the largest diagonal entry.
//   k_tr_project   A = M - Q R^T - R Q^T = Pi M Pi + mu Q Q^T (identity rows for unobserved points and the padding).
//   k_tr_panel / k_tr_trail   blocked right-looking Cholesky, panels of 32 columns, one launch each per panel: every workgroup of the panel launch
//                  factors the 32 x 32 diagonal block in LDS (the same bits everywhere) and solves 64 rows of the panel; the trailing update is
//                  64 x 64 tiles of the lower triangle spread over the device.
//   k_tr_solve     one workgroup: the two triangular solves in blocks of 32, refined, predicted decrease, cost.
// No floating-point atomic, every sum in a fixed order, nothing depends on the launch geometry's timing: two runs give the same bits.
// No dense factorisation on the host and no CPU fallback.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cmath>
#include <cstring>
#include <numeric>
#include <vector>
#include "../../include/vicalib_amd.h"
#include "vc_kutil.hpp"
#include "vc_hostutil.hpp"
#include "vc_target_refine.hpp"

namespace {

using vc::SelRig;
constexpr int kSweepWaves = 2;
// doubles of LDS per wavefront of the sweep: G | Hff | W16 | tmp (gf 6, gc 16) | Wf | Y | gs | yr | Hcc
constexpr int kSweepLds = vc::kSelGramDoubles + 36 + 96 + 24 + 2 * 6 * vc::kSelMaxD + vc::kSelMaxD + 8 + vc::kSelMaxCams * 256;
constexpr int kFrameYs = 6 * vc::kSelMaxD + 8;      // a frame's record: Ys (6 x 64), yr (6)
constexpr int kNStages = 6;

struct TrView {
  SelRig rig;
  int n_frames, P, npad, Ppack, n_corners;
  double lambda;
  // ---- input ----
  const double* poses;          // n_frames x kPoseStride
  const int* frame_view_off;    // n_frames + 1
  const int* view_cam;          // per view
  const int* view_off;          // per view + 1: into the corners
  const int* pt;                // per corner: its target point
  const double* z;              // per corner x 2
  const int* corner_cam;        // per corner
  const int* rec_off;           // n_frames + 1: a frame's (frame, point) records
  const int* rc_off;            // per record + 1: into rc_idx
  const int* rc_idx;            // the corners of a record, by camera
  const int* rec_of;            // n_frames x P: the record of (frame, point) or -1
  const int* pl_off;            // P + 1: the by-point list
  const int* pl_rec;            // its records, frames ascending
  const int* pl_frame;
  const double* points;         // P x 3
  const double* nominal;        // P x 3
  // ---- work ----
  double* corner;               // per corner x kTrCornerStride
  int* corner_ok;
  double* rec;                  // per record x kTrRecStride
  int* rec_nok;
  double* fys;                  // n_frames x kFrameYs
  double* info;                 // n_frames x Ppack
  double* gsf;                  // n_frames x kSelMaxD
  double* fcost;                // n_frames
  int* fstat;                   // n_frames x 3
  double* S;                    // npad x npad
  double* Sds;                  // npad x kSelMaxD, then Z
  double* gd;                   // npad
  double* U;                    // kSelMaxD x kSelMaxD
  double* cscale;               // kSelMaxD
  double* zg;                   // kSelMaxD
  double* Q;                    // 7 x npad
  double* V;                    // 7 x npad, then R
  double* pe;                   // npad: Pi (points - nominal)
  double* rhs;                  // npad: Pi b
  double* xv;                   // npad
  double* Ldiag;                // npad / 32 x 32 x 32
  int* live;                    // npad
  int* pstat;                   // P
  int* pcorners;                // P
  double* sc;                   // [0] mu, [1] top, [2] cost, [3] predicted decrease
  int* si;                      // [0] singular, [1] gauge rank, [2] observed points
  double* refined;              // P x 3
};

template <int MODEL>
__device__ __forceinline__ void view_sweep(const TrView& v, const vc::TileXf& x, const double* K, const vc::ModelPre& pre, const double* Rck, int flags, int o0, int o1,
                                           int lane, double* G, int* corners, int* behind, double* cost) {
  constexpr int NA = vc::sel_nacc(MODEL), NU = vc::sel_nu(MODEL);
  double acc[NA], accg[NU];
#pragma unroll
  for (int a = 0; a < NA; ++a) acc[a] = 0.0;
#pragma unroll
  for (int a = 0; a < NU; ++a) accg[a] = 0.0;
  int ok = 0, bad = 0;
  double c2 = 0.0;
#pragma unroll 1
  for (int o = o0 + lane; o < o1; o += 64) {
    double r0[vc::kUCols], r1[vc::kUCols], r[2];
    const double* pw = v.points + 3 * (size_t)v.pt[o];
    const double p[3] = {pw[0], pw[1], pw[2]};
    const double z[2] = {v.z[2 * (size_t)o], v.z[2 * (size_t)o + 1]};
    double* out = v.corner + (size_t)o * vc::kTrCornerStride;
    if (vc::tr_corner_rows<MODEL>(x, K, pre, p, z, r0, r1, r)) {
      vc::sel_gram_add<MODEL>(r0, r1, acc);
      vc::tr_grad_add<MODEL>(r0, r1, r[0], r[1], accg);
      vc::tr_corner_record<MODEL>(r0, r1, r, Rck, x.Rcw, flags, out);
      v.corner_ok[o] = 1;
      c2 += r[0] * r[0] + r[1] * r[1];
      ++ok;
    } else { vc::tr_corner_zero(out); v.corner_ok[o] = 0; ++bad; }
  }
#pragma unroll
  for (int a = 0; a < NA; ++a) acc[a] = vc::wave_allsum(acc[a]);
#pragma unroll
  for (int a = 0; a < NU; ++a) accg[a] = vc::wave_allsum(accg[a]);
  *corners = vc::wave_allsum(ok);
  *behind = vc::wave_allsum(bad);
  *cost = vc::wave_allsum(c2);
  if (lane == 0) { vc::sel_gram_expand<MODEL>(acc, G); vc::tr_grad_place<MODEL>(accg, G); }
}

__global__ __launch_bounds__(64 * kSweepWaves) void k_tr_sweep(TrView v) {
  __shared__ double s_all[kSweepWaves][kSweepLds];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int f = blockIdx.x * kSweepWaves + wave;
  if (f >= v.n_frames) return;                                    // (wave-uniform; no workgroup barrier below)
  double* G = s_all[wave];
  double* Hff = G + vc::kSelGramDoubles;
  double* W16 = Hff + 36;
  double* tmp = W16 + 96;
  double* Wf = tmp + 24;                                          // 6 x kSelMaxD
  double* Y = Wf + 6 * vc::kSelMaxD;                              // 6 x kSelMaxD
  double* gs = Y + 6 * vc::kSelMaxD;                              // kSelMaxD
  double* yr = gs + vc::kSelMaxD;                                 // 6 (8)
  double* Hcc = yr + 8;                                           // per camera 16 x 16
  const SelRig& rig = v.rig;
  const int D = rig.D;
  for (int k = lane; k < 6 * vc::kSelMaxD; k += 64) Wf[k] = 0.0;
  gs[lane] = 0.0;
  if (lane < 36) Hff[lane] = 0.0;
  if (lane < 24) tmp[lane] = 0.0;
  vc::wave_lds_sync_local();
  unsigned seen = 0;
  int corners = 0, behind = 0;
  double cost = 0.0;
  const double* T_wk = v.poses + (size_t)f * vc::kPoseStride;
  for (int t = v.frame_view_off[f]; t < v.frame_view_off[f + 1]; ++t) {
    const int c = v.view_cam[t];
    const double* cam = rig.cam + c * vc::kCamStride;
    vc::TileXf x;
    double K[10], Rck[9];
    vc::view_setup(T_wk, cam, &x, K);
    vc::quat_to_R(cam, Rck);
    vc::ModelPre pre;
    vc::model_precompute(rig.model[c], K, &pre);
    int n_ok = 0, n_bad = 0;
    double c2 = 0.0;
    vc::with_model(rig.model[c], [&](auto m) {
      view_sweep<decltype(m)::value>(v, x, K, pre, Rck, rig.flags[c], v.view_off[t], v.view_off[t + 1], lane, G, &n_ok, &n_bad, &c2);
    });
    corners += n_ok; behind += n_bad; cost += c2;
    if (n_ok == 0) { vc::wave_lds_sync_local(); continue; }
    vc::wave_lds_sync_local();
    if (lane == 0) vc::sel_view_blocks(G, cam, rig.model[c], rig.flags[c], Hff, W16, Hcc + c * 256, tmp);
    vc::wave_lds_sync_local();
    if (lane < rig.ncols[c]) {
      for (int r = 0; r < 6; ++r) Wf[r * vc::kSelMaxD + rig.col0[c] + lane] = W16[r * vc::kUCols + lane];
      gs[rig.col0[c] + lane] = tmp[6 + lane];
    }
    seen |= 1u << c;
    vc::wave_lds_sync_local();
  }
  double L[36], dinv[6];
#pragma unroll
  for (int k = 0; k < 36; ++k) L[k] = Hff[k];
  const bool chol_ok = corners >= 4 && vc::sel_chol6(L, dinv);
  const int status = vc::sel_frame_status(corners, behind, chol_ok);
  if (lane == 0) { v.fstat[3 * f] = status; v.fstat[3 * f + 1] = corners; v.fstat[3 * f + 2] = behind; v.fcost[f] = cost; }
  double* out = v.info + (size_t)f * v.Ppack;
  double* fy = v.fys + (size_t)f * kFrameYs;
  if (!vc::sel_usable(status)) {
    for (int e = lane; e < v.Ppack; e += 64) out[e] = 0.0;
    v.gsf[(size_t)f * vc::kSelMaxD + lane] = 0.0;
    for (int e = lane; e < kFrameYs; e += 64) fy[e] = 0.0;
    return;
  }
  if (lane < D) vc::sel_schur_col(L, dinv, Wf, vc::kSelMaxD, lane, Y + lane, vc::kSelMaxD);
  if (lane == 0) vc::sel_schur_col(L, dinv, tmp, 1, 0, yr, 1);
  vc::wave_lds_sync_local();
  for (int i = 0; i < D; ++i) {
    const int j = i + lane;
    if (j >= D) continue;
    const int ci = vc::sel_col_cam(rig, i), cj = vc::sel_col_cam(rig, j);
    const double hss = (ci == cj && ((seen >> ci) & 1u)) ? Hcc[ci * 256 + (i - rig.col0[ci]) * vc::kUCols + (j - rig.col0[ci])] : 0.0;
    out[vc::sel_pack_idx(i, j, D)] = vc::sel_info_entry(hss, Y, vc::kSelMaxD, i, j);
  }
  {
    double g = 0.0;
    if (lane < D) { g = gs[lane]; for (int k = 0; k < 6; ++k) g -= Y[k * vc::kSelMaxD + lane] * yr[k]; }
    v.gsf[(size_t)f * vc::kSelMaxD + lane] = g;
    for (int k = 0; k < 6; ++k) fy[k * vc::kSelMaxD + lane] = lane < D ? Y[k * vc::kSelMaxD + lane] : 0.0;
    if (lane < 8) fy[6 * vc::kSelMaxD + lane] = lane < 6 ? yr[lane] : 0.0;
  }
  vc::wave_lds_sync();                                            // (the corners' records, written by other lanes of this wavefront, are read below)
#pragma unroll 1
  for (int e = v.rec_off[f] + lane; e < v.rec_off[f + 1]; e += 64) {
    double rec[vc::kTrRecStride];
#pragma unroll
    for (int k = 0; k < vc::kTrRecStride; ++k) rec[k] = 0.0;
    int nok = 0;
    for (int q = v.rc_off[e]; q < v.rc_off[e + 1]; ++q) {
      const int o = v.rc_idx[q];
      vc::tr_record_add(v.corner + (size_t)o * vc::kTrCornerStride, rec);
      nok += v.corner_ok[o];
    }
    vc::tr_record_solve(L, dinv, rec);
    double* dst = v.rec + (size_t)e * vc::kTrRecStride;
#pragma unroll
    for (int k = 0; k < vc::kTrRecStride; ++k) dst[k] = rec[k];
    v.rec_nok[e] = nok;
  }
}

__global__ __launch_bounds__(256) void k_tr_assemble(TrView v) {
  const int p = blockIdx.x, chunk = blockIdx.y, tid = threadIdx.x;
  const int n_chunks = gridDim.y - 1;
  const int k0 = v.pl_off[p], k1 = v.pl_off[p + 1];
  if (chunk < n_chunks) {
    const int q = chunk * 256 + tid;
    if (q >= v.P) return;
    double acc[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) acc[k] = 0.0;
    for (int k = k0; k < k1; ++k) {
      const int f = v.pl_frame[k];
      if (!vc::sel_usable(v.fstat[3 * f])) continue;
      const int eb = v.rec_of[(size_t)f * v.P + q];
      if (eb < 0) continue;
      const double* ra = v.rec + (size_t)v.pl_rec[k] * vc::kTrRecStride;
      const double* rb = v.rec + (size_t)eb * vc::kTrRecStride;
      if (q == p)
        for (int e = 0; e < 9; ++e) acc[e] += ra[vc::kTrRecP + e];
      vc::tr_pair_sub(ra + vc::kTrRecY, rb + vc::kTrRecY, acc);
    }
    for (int a = 0; a < 3; ++a)
      for (int b = 0; b < 3; ++b) v.S[(size_t)(3 * p + a) * v.npad + 3 * q + b] = acc[a * 3 + b];
    return;
  }
  const SelRig& rig = v.rig;
  if (tid < rig.D) {                                               // the columns of s
    const int c = vc::sel_col_cam(rig, tid), jc = tid - rig.col0[c];
    double acc[3] = {0.0, 0.0, 0.0};
    for (int k = k0; k < k1; ++k) {
      const int f = v.pl_frame[k];
      if (!vc::sel_usable(v.fstat[3 * f])) continue;
      const int e = v.pl_rec[k];
      for (int q = v.rc_off[e]; q < v.rc_off[e + 1]; ++q) {
        const int o = v.rc_idx[q];
        if (v.corner_cam[o] != c) continue;
        const double* cr = v.corner + (size_t)o * vc::kTrCornerStride + vc::kTrCornerC;
        for (int a = 0; a < 3; ++a) acc[a] += cr[a * vc::kUCols + jc];
      }
      const double* Ya = v.rec + (size_t)e * vc::kTrRecStride + vc::kTrRecY;
      const double* ys = v.fys + (size_t)f * kFrameYs + tid;
      for (int a = 0; a < 3; ++a) acc[a] -= vc::tr_y_dot(Ya, a, ys, vc::kSelMaxD);
    }
    for (int a = 0; a < 3; ++a) v.Sds[(size_t)(3 * p + a) * vc::kSelMaxD + tid] = acc[a];
  } else if (tid == 64) {                                          // the gradient
    double acc[3] = {0.0, 0.0, 0.0};
    for (int k = k0; k < k1; ++k) {
      const int f = v.pl_frame[k];
      if (!vc::sel_usable(v.fstat[3 * f])) continue;
      const double* ra = v.rec + (size_t)v.pl_rec[k] * vc::kTrRecStride;
      const double* yr = v.fys + (size_t)f * kFrameYs + 6 * vc::kSelMaxD;
      for (int a = 0; a < 3; ++a) acc[a] += ra[vc::kTrRecG + a] - vc::tr_y_dot(ra + vc::kTrRecY, a, yr, 1);
    }
    for (int a = 0; a < 3; ++a) v.gd[3 * p + a] = -acc[a];
  } else if (tid == 65) {                                          // the point's usable corners
    int n = 0;
    for (int k = k0; k < k1; ++k)
      if (vc::sel_usable(v.fstat[3 * v.pl_frame[k]])) n += v.rec_nok[v.pl_rec[k]];
    v.pcorners[p] = n;
    v.pstat[p] = n > 0 ? vc::kTrPointOk : vc::kTrPointUnobserved;
  }
}

// packed entry e -> (i, j), i <= j
__device__ __forceinline__ void unpack_idx(int e, int D, int* i, int* j) {
  int r = 0;
  while (e >= D - r) { e -= D - r; ++r; }
  *i = r; *j = r + e;
}

__global__ __launch_bounds__(256) void k_tr_shared(TrView v) {
  __shared__ double M[vc::kSelMaxD * vc::kSelMaxD];
  __shared__ double cs[vc::kSelMaxD], g[vc::kSelMaxD];
  const int tid = threadIdx.x, D = v.rig.D;
  for (int e = tid; e < v.Ppack; e += 256) {
    int i, j;
    unpack_idx(e, D, &i, &j);
    double s = 0.0;
    for (int f = 0; f < v.n_frames; ++f)
      if (vc::sel_usable(v.fstat[3 * f])) s += v.info[(size_t)f * v.Ppack + e];
    M[i * D + j] = s;
  }
  if (tid < D) {
    double s = 0.0;
    for (int f = 0; f < v.n_frames; ++f)
      if (vc::sel_usable(v.fstat[3 * f])) s += v.gsf[(size_t)f * vc::kSelMaxD + tid];
    g[tid] = -s;                                                   // (g_s = -(J_s^T r - Y_s^T y_r))
  }
  __syncthreads();
  if (tid < D) cs[tid] = vc::sel_scale(M[tid * D + tid]);
  __syncthreads();
  for (int e = tid; e < v.Ppack; e += 256) {
    int i, j;
    unpack_idx(e, D, &i, &j);
    M[i * D + j] = vc::sel_scaled(M[i * D + j], cs[i], cs[j]) + (i == j ? vc::kTrPriorS : 0.0);
  }
  __syncthreads();
  for (int k = 0; k + 1 < D; ++k) {
    if (tid > k && tid < D) vc::sel_chol_step(M, D, k, tid);
    __syncthreads();
  }
  if (tid < D) {
    for (int i = 0; i <= tid; ++i) v.U[i * vc::kSelMaxD + tid] = M[i * D + tid];
    v.cscale[tid] = cs[tid];
    if (!(M[tid * D + tid] > 0.0)) v.si[0] = vc::kTrSingular;
  }
  if (tid == 0) {                                                  // z_g = U^-T (c o g_s), times sqrt(pivot)
    for (int k = 0; k < D; ++k) cs[k] = cs[k] * g[k];
    for (int k = 0; k < D; ++k) g[k] = vc::tr_fwd_entry(M, D, k, cs[k], g);
    for (int k = 0; k < D; ++k) v.zg[k] = g[k] * sqrt(M[k * D + k]);
  }
}

__global__ __launch_bounds__(64) void k_tr_zrows(TrView v) {
  const int i = blockIdx.x * 64 + threadIdx.x, D = v.rig.D;
  if (i >= 3 * v.P) return;
  double* row = v.Sds + (size_t)i * vc::kSelMaxD;
  for (int k = 0; k < D; ++k) row[k] = vc::tr_fwd_entry(v.U, vc::kSelMaxD, k, v.cscale[k] * row[k], row);
  for (int k = 0; k < D; ++k) row[k] = row[k] * sqrt(v.U[k * vc::kSelMaxD + k]);
}

__global__ __launch_bounds__(256) void k_tr_rank(TrView v) {
  const int i = blockIdx.y * 16 + (threadIdx.x >> 4), j = blockIdx.x * 16 + (threadIdx.x & 15), n = 3 * v.P, D = v.rig.D;
  if (i >= n || j >= n) return;
  const double* zi = v.Sds + (size_t)i * vc::kSelMaxD;
  const double* zj = v.Sds + (size_t)j * vc::kSelMaxD;
  double s = 0.0;
  for (int k = 0; k < D; ++k) s += zi[k] * zj[k];
  v.S[(size_t)i * v.npad + j] -= s;
  if (j == 0) {
    double t = 0.0;
    for (int k = 0; k < D; ++k) t += zi[k] * v.zg[k];
    v.gd[i] -= t;
  }
}

// the sum of one value per thread over a workgroup of 256 in a fixed order; the result in every thread
__device__ __forceinline__ double block_sum(double x, double* sh) {
  const int tid = threadIdx.x;
  sh[tid] = x;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if (tid < s) sh[tid] += sh[tid + s];
    __syncthreads();
  }
  const double r = sh[0];
  __syncthreads();
  return r;
}
__device__ __forceinline__ double block_max(double x, double* sh) {
  const int tid = threadIdx.x;
  sh[tid] = x;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if (tid < s) sh[tid] = sh[tid] > sh[tid + s] ? sh[tid] : sh[tid + s];
    __syncthreads();
  }
  const double r = sh[0];
  __syncthreads();
  return r;
}
__device__ __forceinline__ double strided_dot(const double* a, const double* b, int n, double* sh) {
  double s = 0.0;
  for (int i = threadIdx.x; i < n; i += 256) s += a[i] * b[i];
  return block_sum(s, sh);
}

__global__ __launch_bounds__(256) void k_tr_gauge(TrView v) {
  __shared__ double sh[256];
  const int tid = threadIdx.x, n = 3 * v.P, npad = v.npad;
  double cnt = 0.0, cx[3] = {0.0, 0.0, 0.0};
  for (int i = tid; i < npad; i += 256) v.live[i] = (i < n && v.pstat[i / 3] == vc::kTrPointOk) ? 1 : 0;
  for (int p = tid; p < v.P; p += 256)
    if (v.pstat[p] == vc::kTrPointOk) { cnt += 1.0; for (int a = 0; a < 3; ++a) cx[a] += v.nominal[3 * p + a]; }
  const double n_obs = block_sum(cnt, sh);
  double cen[3];
  for (int a = 0; a < 3; ++a) cen[a] = block_sum(cx[a], sh) / (n_obs > 0.0 ? n_obs : 1.0);
  __syncthreads();                                                 // (live is read by other threads below)
  int rank = 0;
  for (int c = 0; c < vc::kTrGaugeCols; ++c) {
    double* q = v.Q + (size_t)rank * npad;
    for (int i = tid; i < npad; i += 256) {
      double x = 0.0;
      if (v.live[i]) {
        const int p = i / 3;
        const double u[3] = {v.nominal[3 * p] - cen[0], v.nominal[3 * p + 1] - cen[1], v.nominal[3 * p + 2] - cen[2]};
        x = vc::tr_gauge_entry(c, i - 3 * p, u);
      }
      q[i] = x;
    }
    __syncthreads();
    const double before = sqrt(strided_dot(q, q, npad, sh));
    for (int k = 0; k < rank; ++k) {
      const double* qk = v.Q + (size_t)k * npad;
      const double d = strided_dot(qk, q, npad, sh);
      for (int i = tid; i < npad; i += 256) q[i] -= d * qk[i];
      __syncthreads();
    }
    const double after = sqrt(strided_dot(q, q, npad, sh));
    if (vc::tr_gauge_keep(after, before)) {
      for (int i = tid; i < npad; i += 256) q[i] = q[i] / after;
      ++rank;
    }
    __syncthreads();
  }
  for (int c = rank; c < vc::kTrGaugeCols; ++c)
    for (int i = tid; i < npad; i += 256) v.Q[(size_t)c * npad + i] = 0.0;
  // Pi (points - nominal)
  for (int i = tid; i < npad; i += 256) v.pe[i] = v.live[i] ? v.points[i] - v.nominal[i] : 0.0;
  __syncthreads();
  double t[vc::kTrGaugeCols];
  for (int c = 0; c < vc::kTrGaugeCols; ++c) t[c] = strided_dot(v.Q + (size_t)c * npad, v.pe, npad, sh);
  for (int i = tid; i < npad; i += 256) {
    double x = v.pe[i];
    for (int c = 0; c < vc::kTrGaugeCols; ++c) x -= v.Q[(size_t)c * npad + i] * t[c];
    v.pe[i] = v.live[i] ? x : 0.0;
  }
  __syncthreads();
  // Pi b,  b = g - lambda Pi (points - nominal)
  for (int i = tid; i < npad; i += 256) v.rhs[i] = v.live[i] ? v.gd[i] - v.lambda * v.pe[i] : 0.0;
  __syncthreads();
  for (int c = 0; c < vc::kTrGaugeCols; ++c) t[c] = strided_dot(v.Q + (size_t)c * npad, v.rhs, npad, sh);
  double tr = 0.0;
  for (int i = tid; i < npad; i += 256) {
    double x = v.rhs[i];
    for (int c = 0; c < vc::kTrGaugeCols; ++c) x -= v.Q[(size_t)c * npad + i] * t[c];
    v.rhs[i] = v.live[i] ? x : 0.0;
    if (v.live[i]) tr += v.S[(size_t)i * npad + i] + v.lambda;
  }
  const double trace = block_sum(tr, sh);
  if (tid == 0) {
    v.sc[0] = trace / (3.0 * (n_obs > 0.0 ? n_obs : 1.0));
    v.si[1] = rank; v.si[2] = (int)n_obs;
    if (!(n_obs > 0.0)) v.si[0] = vc::kTrSingular;
  }
}

__global__ __launch_bounds__(64) void k_tr_mq(TrView v) {
  const int i = blockIdx.x * 64 + threadIdx.x, npad = v.npad;
  double acc[vc::kTrGaugeCols];
  for (int c = 0; c < vc::kTrGaugeCols; ++c) acc[c] = 0.0;
  if (v.live[i])
    for (int j = 0; j < 3 * v.P; ++j) {
      if (!v.live[j]) continue;
      const double m = v.S[(size_t)j * npad + i] + (i == j ? v.lambda : 0.0);
      for (int c = 0; c < vc::kTrGaugeCols; ++c) acc[c] += m * v.Q[(size_t)c * npad + j];
    }
  for (int c = 0; c < vc::kTrGaugeCols; ++c) v.V[(size_t)c * npad + i] = acc[c];
}

__global__ __launch_bounds__(256) void k_tr_gauge2(TrView v) {
  __shared__ double sh[256];
  __shared__ double G7[vc::kTrGaugeCols * vc::kTrGaugeCols];
  const int tid = threadIdx.x, npad = v.npad;
  const double mu = v.sc[0];
  for (int a = 0; a < vc::kTrGaugeCols; ++a)
    for (int b = 0; b < vc::kTrGaugeCols; ++b) {
      const double s = strided_dot(v.Q + (size_t)a * npad, v.V + (size_t)b * npad, npad, sh);
      if (tid == 0) G7[a * vc::kTrGaugeCols + b] = s;
    }
  __syncthreads();
  double top = 0.0;
  for (int i = tid; i < npad; i += 256) {
    double q[vc::kTrGaugeCols], dd = 0.0;
    for (int a = 0; a < vc::kTrGaugeCols; ++a) q[a] = v.Q[(size_t)a * npad + i];
    for (int c = 0; c < vc::kTrGaugeCols; ++c) {
      double s = 0.0;
      for (int a = 0; a < vc::kTrGaugeCols; ++a) s += q[a] * (0.5 * (G7[a * vc::kTrGaugeCols + c] + G7[c * vc::kTrGaugeCols + a]) + (a == c ? mu : 0.0));
      const double r = v.V[(size_t)c * npad + i] - 0.5 * s;
      v.V[(size_t)c * npad + i] = r;
      dd += q[c] * r;
    }
    if (v.live[i]) { const double d = v.S[(size_t)i * npad + i] + v.lambda - 2.0 * dd; top = d > top ? d : top; }
  }
  const double t = block_max(top, sh);
  if (tid == 0) v.sc[1] = t;
}

__global__ __launch_bounds__(256) void k_tr_project(TrView v) {
  const int i = blockIdx.y * 16 + (threadIdx.x >> 4), j = blockIdx.x * 16 + (threadIdx.x & 15), npad = v.npad;
  double a = i == j ? 1.0 : 0.0;
  if (v.live[i] && v.live[j]) {
    double s = 0.0;
    for (int c = 0; c < vc::kTrGaugeCols; ++c) s += v.Q[(size_t)c * npad + i] * v.V[(size_t)c * npad + j] + v.V[(size_t)c * npad + i] * v.Q[(size_t)c * npad + j];
    a = v.S[(size_t)i * npad + j] + (i == j ? v.lambda : 0.0) - s;
  }
  v.S[(size_t)i * npad + j] = a;
}

// the panel at column k0: every workgroup factors the diagonal block (the same bits), workgroup 0 keeps the factor, workgroup b >= 1 solves rows
// k0 + 32 + 64 (b - 1) .. of the panel
__global__ __launch_bounds__(64) void k_tr_panel(TrView v, int k0) {
  constexpr int NB = vc::kTrNB;
  __shared__ double Ld[NB][NB + 1];
  __shared__ double X[NB][64];
  if (v.si[0]) return;      // (workgroup 0 of THIS launch may be setting the word: a workgroup that misses it only writes into S, which a singular result never reads back)
  const int tid = threadIdx.x, npad = v.npad;
  const double top = v.sc[1];
  for (int idx = tid; idx < NB * NB; idx += 64) { const int r = idx >> 5, c = idx & 31; Ld[r][c] = v.S[(size_t)(k0 + r) * npad + k0 + c]; }
  __syncthreads();
  int bad = 0;
  for (int j = 0; j < NB; ++j) {
    const double d = Ld[j][j];
    if (v.live[k0 + j] && !vc::tr_pivot_ok(d, top)) bad = 1;
    const double l = sqrt(d);
    __syncthreads();
    if (tid > j && tid < NB) Ld[tid][j] = Ld[tid][j] / l;
    if (tid == j) Ld[j][j] = l;
    __syncthreads();
    if (tid > j && tid < NB)
      for (int c = j + 1; c <= tid; ++c) Ld[tid][c] -= Ld[tid][j] * Ld[c][j];
    __syncthreads();
  }
  if (blockIdx.x == 0) {
    double* dst = v.Ldiag + (size_t)(k0 / NB) * NB * NB;
    for (int idx = tid; idx < NB * NB; idx += 64) { const int r = idx >> 5, c = idx & 31; dst[idx] = c <= r ? Ld[r][c] : 0.0; }
    if (bad && tid == 0) v.si[0] = vc::kTrSingular;
    return;
  }
  const int i = k0 + NB + (blockIdx.x - 1) * 64 + tid;
  if (i >= npad) return;
  double* row = v.S + (size_t)i * npad + k0;
  for (int c = 0; c < NB; ++c) X[c][tid] = row[c];
  for (int c = 0; c < NB; ++c) {
    double s = X[c][tid];
    for (int m = 0; m < c; ++m) s -= X[m][tid] * Ld[c][m];
    s = s / Ld[c][c];
    X[c][tid] = s;
    row[c] = s;
  }
}

// the trailing update behind the panel at k0: 64 x 64 tiles of the lower triangle, A22 -= L21 L21^T
__global__ __launch_bounds__(256) void k_tr_trail(TrView v, int k0) {
  constexpr int NB = vc::kTrNB;
  __shared__ double Li[64][NB + 1], Lj[64][NB + 1];
  if (v.si[0] || blockIdx.x > blockIdx.y) return;
  const int tid = threadIdx.x, npad = v.npad;
  const int i0 = k0 + NB + blockIdx.y * 64, j0 = k0 + NB + blockIdx.x * 64;
  for (int idx = tid; idx < 64 * NB; idx += 256) {
    const int r = idx >> 5, c = idx & 31;
    Li[r][c] = i0 + r < npad ? v.S[(size_t)(i0 + r) * npad + k0 + c] : 0.0;
    Lj[r][c] = j0 + r < npad ? v.S[(size_t)(j0 + r) * npad + k0 + c] : 0.0;
  }
  __syncthreads();
  const int ty = tid >> 4, tx = tid & 15;
  double acc[4][4];
#pragma unroll
  for (int a = 0; a < 4; ++a)
#pragma unroll
    for (int b = 0; b < 4; ++b) acc[a][b] = 0.0;
#pragma unroll 4
  for (int c = 0; c < NB; ++c) {
    double li[4], lj[4];
#pragma unroll
    for (int a = 0; a < 4; ++a) { li[a] = Li[ty + 16 * a][c]; lj[a] = Lj[tx + 16 * a][c]; }
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
      for (int b = 0; b < 4; ++b) acc[a][b] += li[a] * lj[b];
  }
#pragma unroll
  for (int a = 0; a < 4; ++a)
#pragma unroll
    for (int b = 0; b < 4; ++b) {
      const int i = i0 + ty + 16 * a, j = j0 + tx + 16 * b;
      if (i < npad && j <= i) v.S[(size_t)i * npad + j] -= acc[a][b];
    }
}

__global__ __launch_bounds__(256) void k_tr_solve(TrView v) {
  constexpr int NB = vc::kTrNB;
  __shared__ double sh[256];
  __shared__ double Ld[NB][NB + 1];
  __shared__ double xs[NB];
  if (v.si[0]) return;
  const int tid = threadIdx.x, npad = v.npad, nblk = npad / NB;
  for (int i = tid; i < npad; i += 256) v.xv[i] = v.rhs[i];
  __syncthreads();
  for (int kb = 0; kb < nblk; ++kb) {                              // L y = Pi b
    const int k0 = kb * NB;
    for (int idx = tid; idx < NB * NB; idx += 256) Ld[idx >> 5][idx & 31] = v.Ldiag[(size_t)kb * NB * NB + idx];
    if (tid < NB) xs[tid] = v.xv[k0 + tid];
    __syncthreads();
    if (tid == 0)
      for (int r = 0; r < NB; ++r) {
        double s = xs[r];
        for (int c = 0; c < r; ++c) s -= Ld[r][c] * xs[c];
        xs[r] = s / Ld[r][r];
      }
    __syncthreads();
    if (tid < NB) v.xv[k0 + tid] = xs[tid];
    for (int i = k0 + NB + tid; i < npad; i += 256) {
      const double* row = v.S + (size_t)i * npad + k0;
      double s = v.xv[i];
      for (int c = 0; c < NB; ++c) s -= row[c] * xs[c];
      v.xv[i] = s;
    }
    __syncthreads();
  }
  for (int kb = nblk - 1; kb >= 0; --kb) {                         // L^T d = y
    const int k0 = kb * NB;
    for (int idx = tid; idx < NB * NB; idx += 256) Ld[idx >> 5][idx & 31] = v.Ldiag[(size_t)kb * NB * NB + idx];
    if (tid < NB) xs[tid] = v.xv[k0 + tid];
    __syncthreads();
    if (tid == 0)
      for (int r = NB - 1; r >= 0; --r) {
        double s = xs[r];
        for (int c = r + 1; c < NB; ++c) s -= Ld[c][r] * xs[c];
        xs[r] = s / Ld[r][r];
      }
    __syncthreads();
    if (tid < NB) v.xv[k0 + tid] = xs[tid];
    for (int i = tid; i < k0; i += 256) {
      double s = v.xv[i];
      for (int c = 0; c < NB; ++c) s -= v.S[(size_t)(k0 + c) * npad + i] * xs[c];
      v.xv[i] = s;
    }
    __syncthreads();
  }
  double pd = 0.0;
  for (int i = tid; i < 3 * v.P; i += 256) {
    pd += v.xv[i] * v.rhs[i];
    v.refined[i] = v.live[i] ? v.nominal[i] + v.pe[i] + v.xv[i] : v.points[i];
  }
  const double pred = block_sum(pd, sh);
  double c = 0.0;
  for (int f = tid; f < v.n_frames; f += 256)
    if (vc::sel_usable(v.fstat[3 * f])) c += v.fcost[f];
  const double cost = block_sum(c, sh);
  if (tid == 0) { v.sc[2] = 0.5 * cost; v.sc[3] = 0.5 * pred; }
}

struct TrArgs {
  int n_cameras; const int* model; const double* params; const double* T_ck; const int* cam_flags;
  int n_frames; const double* T_wk;
  int n_tiles; const int* tile_frame; const int* tile_cam; const long long* tile_off; const int* point_id; const double* p_c;
  const double* points; const double* nominal; int n_points; double lambda;
};

// VC_OK, VC_ERR_BAD_ARG or VC_ERR_UNSUPPORTED, before any device call; fills the rig
int check_args(const TrArgs& a, SelRig* rig) {
  if (a.n_cameras < 1 || a.n_cameras > vc::kSelMaxCams || !a.model || !a.params || !a.T_ck || !a.cam_flags || a.n_frames < 1 || !a.T_wk || a.n_tiles < 0 ||
      !a.points || !a.nominal || (a.n_tiles > 0 && (!a.tile_frame || !a.tile_cam || !a.tile_off)) || !vc::sel_prior_ok(a.lambda) || a.n_points < vc::kTrMinPoints)
    return VC_ERR_BAD_ARG;
  std::memset(rig, 0, sizeof(*rig));
  rig->n_cams = a.n_cameras;
  for (int c = 0; c < a.n_cameras; ++c) {
    const int nk = vc::model_nk(a.model[c]);
    if (nk < 0 || (a.cam_flags[c] & ~7) != 0) return VC_ERR_BAD_ARG;
    for (int k = 0; k < nk; ++k) if (!std::isfinite(a.params[10 * c + k])) return VC_ERR_BAD_ARG;
    for (int k = 0; k < 7; ++k) if (!std::isfinite(a.T_ck[7 * c + k])) return VC_ERR_BAD_ARG;
    rig->model[c] = a.model[c]; rig->flags[c] = a.cam_flags[c];
    std::memcpy(rig->cam + c * vc::kCamStride, a.T_ck + 7 * c, 56);
    std::memcpy(rig->cam + c * vc::kCamStride + vc::kCamK, a.params + 10 * c, (size_t)nk * 8);
  }
  for (size_t k = 0; k < 7 * (size_t)a.n_frames; ++k) if (!std::isfinite(a.T_wk[k])) return VC_ERR_BAD_ARG;
  if (a.n_tiles > 0) {
    if (a.tile_off[0] < 0) return VC_ERR_BAD_ARG;
    for (int t = 0; t < a.n_tiles; ++t)
      if (a.tile_frame[t] < 0 || a.tile_frame[t] >= a.n_frames || a.tile_cam[t] < 0 || a.tile_cam[t] >= a.n_cameras || a.tile_off[t + 1] < a.tile_off[t]) return VC_ERR_BAD_ARG;
    const long long m = a.tile_off[a.n_tiles];
    if (m > 0x3fffffff) return VC_ERR_BAD_ARG;
    if (m > a.tile_off[0] && (!a.point_id || !a.p_c)) return VC_ERR_BAD_ARG;
    for (long long o = a.tile_off[0]; o < m; ++o)
      if (a.point_id[o] < 0 || a.point_id[o] >= a.n_points || !std::isfinite(a.p_c[2 * o]) || !std::isfinite(a.p_c[2 * o + 1])) return VC_ERR_BAD_ARG;
  }
  for (int k = 0; k < 3 * a.n_points; ++k) if (!std::isfinite(a.points[k]) || !std::isfinite(a.nominal[k])) return VC_ERR_BAD_ARG;
  if (a.n_points > vc::kTrMaxPoints || a.n_frames > vc::kTrMaxFrames) return VC_ERR_UNSUPPORTED;
  if (!vc::sel_layout(rig)) return VC_ERR_UNSUPPORTED;
  return VC_OK;
}

struct TrOut {
  double* refined; int* point_status; int* point_corners; int* frame_status; int* gauge_rank; int* result_status; double* cost; double* predicted_decrease;
};

int run(int device, const TrArgs& a, const SelRig& rig, const TrOut& out, int time_reps, double* stage_ms) {
  if (vch::open_device(device) != VC_OK) return VC_ERR_NO_DEVICE;
  (void)hipGetLastError();                                         // (an error an earlier call of the process left behind is not this call's)
  const int N = a.n_frames, P = a.n_points, D = rig.D, npad = vc::tr_padded(P), Ppack = vc::sel_pack_len(D);
  // the device image of the input: views ordered by frame, then camera; the corners of a view in the order of arrival
  std::vector<int> o_frame, o_cam, o_pt;
  std::vector<double> o_z;
  for (int t = 0; t < a.n_tiles; ++t)
    for (long long o = a.tile_off[t]; o < a.tile_off[t + 1]; ++o) {
      o_frame.push_back(a.tile_frame[t]); o_cam.push_back(a.tile_cam[t]); o_pt.push_back(a.point_id[o]);
      o_z.push_back(a.p_c[2 * o]); o_z.push_back(a.p_c[2 * o + 1]);
    }
  const size_t M = o_frame.size();
  std::vector<size_t> ord(M);
  std::iota(ord.begin(), ord.end(), (size_t)0);
  std::stable_sort(ord.begin(), ord.end(), [&](size_t x, size_t y) { return o_frame[x] != o_frame[y] ? o_frame[x] < o_frame[y] : o_cam[x] < o_cam[y]; });
  std::vector<int> frame_view_off(N + 1, 0), frame_first(N + 1, 0), view_cam, view_off, pt(M), ccam(M);
  std::vector<double> z(2 * M);
  {
    size_t k = 0;
    for (int f = 0; f < N; ++f) {
      frame_view_off[f] = (int)view_cam.size(); frame_first[f] = (int)k;
      while (k < M && o_frame[ord[k]] == f) {
        const int c = o_cam[ord[k]];
        view_cam.push_back(c); view_off.push_back((int)k);
        while (k < M && o_frame[ord[k]] == f && o_cam[ord[k]] == c) { pt[k] = o_pt[ord[k]]; ccam[k] = c; z[2 * k] = o_z[2 * ord[k]]; z[2 * k + 1] = o_z[2 * ord[k] + 1]; ++k; }
      }
    }
    frame_view_off[N] = (int)view_cam.size(); frame_first[N] = (int)M;
    view_off.push_back((int)M);
  }
  // the (frame, point) records, their corners by camera, the table (frame, point) -> record and the by-point list
  std::vector<int> rec_off(N + 1, 0), rc_off(1, 0), rc_idx, rec_pt, rec_frame, rec_of((size_t)N * P, -1);
  for (int f = 0; f < N; ++f) {
    rec_off[f] = (int)rec_pt.size();
    std::vector<int> idx(frame_first[f + 1] - frame_first[f]);
    std::iota(idx.begin(), idx.end(), frame_first[f]);
    std::stable_sort(idx.begin(), idx.end(), [&](int x, int y) { return pt[x] < pt[y]; });
    for (size_t q = 0; q < idx.size();) {
      const int p = pt[idx[q]];
      rec_of[(size_t)f * P + p] = (int)rec_pt.size();
      rec_pt.push_back(p); rec_frame.push_back(f);
      while (q < idx.size() && pt[idx[q]] == p) rc_idx.push_back(idx[q++]);
      rc_off.push_back((int)rc_idx.size());
    }
  }
  rec_off[N] = (int)rec_pt.size();
  const size_t R = rec_pt.size();
  std::vector<int> pl_off(P + 1, 0), pl_rec(R), pl_frame(R);
  for (size_t e = 0; e < R; ++e) ++pl_off[rec_pt[e] + 1];
  for (int p = 0; p < P; ++p) pl_off[p + 1] += pl_off[p];
  {
    std::vector<int> fill(pl_off.begin(), pl_off.end() - 1);
    for (size_t e = 0; e < R; ++e) { const int k = fill[rec_pt[e]]++; pl_rec[k] = (int)e; pl_frame[k] = rec_frame[e]; }      // (records are in frame order)
  }
  std::vector<double> poses((size_t)N * vc::kPoseStride, 0.0);
  for (int f = 0; f < N; ++f) std::memcpy(&poses[(size_t)f * vc::kPoseStride], a.T_wk + (size_t)f * 7, 56);

  TrView v;
  std::memset(&v, 0, sizeof(v));
  v.rig = rig; v.n_frames = N; v.P = P; v.npad = npad; v.Ppack = Ppack; v.n_corners = (int)M; v.lambda = a.lambda;
  double* d_poses = nullptr; int *d_fvo = nullptr, *d_vc = nullptr, *d_vo = nullptr, *d_pt = nullptr, *d_ccam = nullptr, *d_rec_off = nullptr, *d_rc_off = nullptr,
      *d_rc_idx = nullptr, *d_rec_of = nullptr, *d_pl_off = nullptr, *d_pl_rec = nullptr, *d_pl_frame = nullptr;
  double *d_z = nullptr, *d_points = nullptr, *d_nominal = nullptr;
  size_t zero_from = 0;
  auto carve = [&](vch::Carver q) {
    d_poses = q.take<double>(poses.size());
    d_fvo = q.take<int>(frame_view_off.size()); d_vc = q.take<int>(view_cam.size() + 1); d_vo = q.take<int>(view_off.size()); d_pt = q.take<int>(M + 1);
    d_ccam = q.take<int>(M + 1); d_z = q.take<double>(2 * M + 2);
    d_rec_off = q.take<int>(rec_off.size()); d_rc_off = q.take<int>(rc_off.size()); d_rc_idx = q.take<int>(rc_idx.size() + 1); d_rec_of = q.take<int>(rec_of.size());
    d_pl_off = q.take<int>(pl_off.size()); d_pl_rec = q.take<int>(R + 1); d_pl_frame = q.take<int>(R + 1);
    d_points = q.take<double>(3 * (size_t)P); d_nominal = q.take<double>(3 * (size_t)P);
    zero_from = q.bytes();
    v.corner = q.take<double>((M + 1) * vc::kTrCornerStride); v.corner_ok = q.take<int>(M + 1);
    v.rec = q.take<double>((R + 1) * vc::kTrRecStride); v.rec_nok = q.take<int>(R + 1);
    v.fys = q.take<double>((size_t)N * kFrameYs); v.info = q.take<double>((size_t)N * Ppack + 1); v.gsf = q.take<double>((size_t)N * vc::kSelMaxD);
    v.fcost = q.take<double>(N); v.fstat = q.take<int>((size_t)N * 3);
    v.S = q.take<double>((size_t)npad * npad); v.Sds = q.take<double>((size_t)npad * vc::kSelMaxD); v.gd = q.take<double>(npad);
    v.U = q.take<double>(vc::kSelMaxD * vc::kSelMaxD); v.cscale = q.take<double>(vc::kSelMaxD); v.zg = q.take<double>(vc::kSelMaxD);
    v.Q = q.take<double>((size_t)vc::kTrGaugeCols * npad); v.V = q.take<double>((size_t)vc::kTrGaugeCols * npad);
    v.pe = q.take<double>(npad); v.rhs = q.take<double>(npad); v.xv = q.take<double>(npad);
    v.Ldiag = q.take<double>((size_t)(npad / vc::kTrNB) * vc::kTrNB * vc::kTrNB);
    v.live = q.take<int>(npad); v.pstat = q.take<int>(P); v.pcorners = q.take<int>(P);
    v.sc = q.take<double>(4); v.si = q.take<int>(4);
    v.refined = q.take<double>(3 * (size_t)P);
    return q.bytes();
  };
  unsigned char* d_buf = nullptr;
  const size_t bytes = carve(vch::Carver());
  if (hipMalloc((void**)&d_buf, bytes) != hipSuccess) return VC_ERR_NO_DEVICE;
  carve(vch::Carver(d_buf));
  v.poses = d_poses; v.frame_view_off = d_fvo; v.view_cam = d_vc; v.view_off = d_vo; v.pt = d_pt; v.z = d_z; v.corner_cam = d_ccam;
  v.rec_off = d_rec_off; v.rc_off = d_rc_off; v.rc_idx = d_rc_idx; v.rec_of = d_rec_of; v.pl_off = d_pl_off; v.pl_rec = d_pl_rec; v.pl_frame = d_pl_frame;
  v.points = d_points; v.nominal = d_nominal;
  hipStream_t stream = nullptr;
  auto up = [&](void* dst, const void* src, size_t n) { return n == 0 || hipMemcpyAsync(dst, src, n, hipMemcpyHostToDevice, stream) == hipSuccess; };
  auto down = [&](void* dst, const void* src, size_t n) { return n == 0 || hipMemcpyAsync(dst, src, n, hipMemcpyDeviceToHost, stream) == hipSuccess; };
  bool ok = hipMemsetAsync(d_buf + zero_from, 0, bytes - zero_from, stream) == hipSuccess &&
            up(d_poses, poses.data(), poses.size() * 8) && up(d_fvo, frame_view_off.data(), frame_view_off.size() * 4) && up(d_vc, view_cam.data(), view_cam.size() * 4) &&
            up(d_vo, view_off.data(), view_off.size() * 4) && up(d_pt, pt.data(), M * 4) && up(d_ccam, ccam.data(), M * 4) && up(d_z, z.data(), 2 * M * 8) &&
            up(d_rec_off, rec_off.data(), rec_off.size() * 4) && up(d_rc_off, rc_off.data(), rc_off.size() * 4) && up(d_rc_idx, rc_idx.data(), rc_idx.size() * 4) &&
            up(d_rec_of, rec_of.data(), rec_of.size() * 4) && up(d_pl_off, pl_off.data(), pl_off.size() * 4) && up(d_pl_rec, pl_rec.data(), R * 4) &&
            up(d_pl_frame, pl_frame.data(), R * 4) && up(d_points, a.points, 3 * (size_t)P * 8) && up(d_nominal, a.nominal, 3 * (size_t)P * 8);
  // the stages: 0 sweep, 1 assembly, 2 elimination of s, 3 gauge, 4 factorisation, 5 solve
  auto stage = [&](int s) {
    const unsigned t16 = (unsigned)(npad / 16);
    switch (s) {
      case 0: hipLaunchKernelGGL(k_tr_sweep, dim3((N + kSweepWaves - 1) / kSweepWaves), dim3(64 * kSweepWaves), 0, stream, v); break;
      case 1: hipLaunchKernelGGL(k_tr_assemble, dim3(P, (P + 255) / 256 + 1), dim3(256), 0, stream, v); break;
      case 2:
        if (D > 0) {
          hipLaunchKernelGGL(k_tr_shared, dim3(1), dim3(256), 0, stream, v);
          hipLaunchKernelGGL(k_tr_zrows, dim3((3 * P + 63) / 64), dim3(64), 0, stream, v);
          hipLaunchKernelGGL(k_tr_rank, dim3(t16, t16), dim3(256), 0, stream, v);
        }
        break;
      case 3:
        hipLaunchKernelGGL(k_tr_gauge, dim3(1), dim3(256), 0, stream, v);
        hipLaunchKernelGGL(k_tr_mq, dim3(npad / 64), dim3(64), 0, stream, v);
        hipLaunchKernelGGL(k_tr_gauge2, dim3(1), dim3(256), 0, stream, v);
        hipLaunchKernelGGL(k_tr_project, dim3(t16, t16), dim3(256), 0, stream, v);
        break;
      case 4:
        for (int k0 = 0; k0 < npad; k0 += vc::kTrNB) {
          const int rest = npad - k0 - vc::kTrNB, tiles = (rest + 63) / 64;
          hipLaunchKernelGGL(k_tr_panel, dim3(1 + tiles), dim3(64), 0, stream, v, k0);
          if (tiles > 0) hipLaunchKernelGGL(k_tr_trail, dim3(tiles, tiles), dim3(256), 0, stream, v, k0);
        }
        break;
      default: hipLaunchKernelGGL(k_tr_solve, dim3(1), dim3(256), 0, stream, v); break;
    }
  };
  int si[4] = {0, 0, 0, 0};
  double sc[4] = {0, 0, 0, 0};
  std::vector<double> refined(3 * (size_t)P);
  std::vector<int> pstat(P), pcorners(P), fstat((size_t)N * 3);
  if (ok) {
    for (int s = 0; s < kNStages; ++s) stage(s);
    ok = hipGetLastError() == hipSuccess && down(si, v.si, sizeof(si)) && down(sc, v.sc, sizeof(sc)) && down(refined.data(), v.refined, refined.size() * 8) &&
         down(pstat.data(), v.pstat, (size_t)P * 4) && down(pcorners.data(), v.pcorners, (size_t)P * 4) && down(fstat.data(), v.fstat, fstat.size() * 4);
  }
  ok = hipStreamSynchronize(stream) == hipSuccess && ok;
  if (ok && stage_ms && time_reps > 0) {                            // (the whole step again on the same input: every stage rewrites what it wrote)
    vch::EventSet<kNStages + 1> ev;
    ok = ev.create();
    for (int s = 0; s < kNStages; ++s) stage_ms[s] = 0.0;
    for (int r = 0; ok && r < time_reps; ++r) {
      ok = hipMemsetAsync(v.si, 0, 16, stream) == hipSuccess && hipEventRecord(ev.e[0], stream) == hipSuccess;
      for (int s = 0; ok && s < kNStages; ++s) { stage(s); ok = hipEventRecord(ev.e[s + 1], stream) == hipSuccess; }
      ok = ok && hipEventSynchronize(ev.e[kNStages]) == hipSuccess && hipGetLastError() == hipSuccess;
      for (int s = 0; ok && s < kNStages; ++s) {
        float ms = 0.f;
        ok = hipEventElapsedTime(&ms, ev.e[s], ev.e[s + 1]) == hipSuccess;
        stage_ms[s] += (double)ms / time_reps;
      }
    }
  }
  (void)hipFree(d_buf);
  if (!ok) return VC_ERR_NO_DEVICE;
  std::memcpy(out.point_status, pstat.data(), (size_t)P * 4);
  std::memcpy(out.point_corners, pcorners.data(), (size_t)P * 4);
  std::memcpy(out.frame_status, fstat.data(), fstat.size() * 4);
  *out.gauge_rank = si[1];
  *out.result_status = si[0] ? vc::kTrSingular : vc::kTrOk;
  if (!si[0]) {                                                    // a singular result leaves the caller's values untouched
    std::memcpy(out.refined, refined.data(), refined.size() * 8);
    *out.cost = sc[2]; *out.predicted_decrease = sc[3];
  }
  return VC_OK;
}

}  // namespace

extern "C" int vc_target_refine_batch(int device, int n_cameras, const int* model, const double* params, const double* T_ck, const int* cam_flags, int n_frames,
                                      const double* T_wk, int n_tiles, const int* tile_frame, const int* tile_cam, const long long* tile_off, const int* point_id,
                                      const double* p_c, const double* points, const double* nominal, int n_points, double lambda, double* refined,
                                      int* point_status, int* point_corners, int* frame_status, int* gauge_rank, int* result_status, double* cost,
                                      double* predicted_decrease) {
  if (!refined || !point_status || !point_corners || !frame_status || !gauge_rank || !result_status || !cost || !predicted_decrease) return VC_ERR_BAD_ARG;
  const TrArgs a{n_cameras, model, params, T_ck, cam_flags, n_frames, T_wk, n_tiles, tile_frame, tile_cam, tile_off, point_id, p_c, points, nominal, n_points, lambda};
  SelRig rig;
  const int rc = check_args(a, &rig);
  if (rc != VC_OK) return rc;
  const TrOut out{refined, point_status, point_corners, frame_status, gauge_rank, result_status, cost, predicted_decrease};
  return run(device, a, rig, out, 0, nullptr);
}

extern "C" int vc_time_target_refine_batch(int device, int n_cameras, const int* model, const double* params, const double* T_ck, const int* cam_flags, int n_frames,
                                           const double* T_wk, int n_tiles, const int* tile_frame, const int* tile_cam, const long long* tile_off,
                                           const int* point_id, const double* p_c, const double* points, const double* nominal, int n_points, double lambda,
                                           int reps, double* kernel_ms) {
  if (reps < 1 || !kernel_ms) return VC_ERR_BAD_ARG;
  const TrArgs a{n_cameras, model, params, T_ck, cam_flags, n_frames, T_wk, n_tiles, tile_frame, tile_cam, tile_off, point_id, p_c, points, nominal, n_points, lambda};
  SelRig rig;
  const int rc = check_args(a, &rig);
  if (rc != VC_OK) return rc;
  std::vector<double> refined(3 * (size_t)n_points);
  std::vector<int> pstat(n_points), pcorners(n_points), fstat(3 * (size_t)n_frames);
  int rank = 0, status = 0;
  double cost = 0.0, pred = 0.0;
  const TrOut out{refined.data(), pstat.data(), pcorners.data(), fstat.data(), &rank, &status, &cost, &pred};
  return run(device, a, rig, out, reps, kernel_ms);
}
