// vc_select.hip -- greedy D-optimal selection of the most informative views of a calibration on the GPU (gfx950, wave64, fp64).
//
// A vc_selector holds a rig, candidate frames (poses and (frame, camera) groups of target points) and the result of the last run
// (vc_select.hpp has the arithmetic and the definition).  Nothing is allocated on the device before the first vc_select_run.
//
//   k_select_info    one wavefront per candidate frame, two per workgroup, no workgroup barrier.  Lanes stride over the corners of each view
//                    and keep the upper triangle of the view's Gram block in registers (indices are compile-time constants of the model's
//                    instantiation); wave_allsum per entry; lane 0 expands the block into LDS and runs tile_to_frame_blocks and
//                    cam_block_from_gsum on it; after the last view the 6 x 6 Cholesky (every lane, in registers), lane = column for
//                    L^-1 W, and one store of the packed upper triangle of I_f.  A frame's arithmetic does not depend on its neighbours.
//   k_select_scale   lane = column: the diagonals summed in frame order over the usable frames -> s.
//   k_select_init    thread = packed entry: S_0 = prior I + sum over the start set, S_all = S_0 + sum over every other usable frame, both in
//                    frame order; marks the start set; resets the run's state.
//   k_select_logdet0 one wavefront: the pivots of S_0 (kept: cum refers to them) and of S_all -> total.
//   k_select_gain    one wavefront per frame: S + I~_f expanded into the wave's D x D of LDS, factored in place with lane = column
//                    (sel_chol_step), gain = sum log(p'_k / p_k) against the pivots of S.  Workgroups of as many waves as 64 KB of LDS hold.
//   k_select_pick    one wavefront: argmax (lanes take frames in ascending order, then wave_argmax_low), S += I~_pick, its pivots, cum, the
//                    selected mask and the round's record.
// All rounds are enqueued back to back; the stop conditions live in a device word every later kernel of the run looks at; one copy comes back.
// No floating-point atomic anywhere and no dependence on the launch geometry: two runs give the same bits.  No CPU fallback.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cmath>
#include <cstring>
#include <numeric>
#include <vector>
#include "../../include/vicalib_amd.h"
#include "vc_kutil.hpp"
#include "vc_hostutil.hpp"
#include "vc_select.hpp"

namespace {

using vc::SelRig;
constexpr int kInfoWaves = 2;                                   // wavefronts (frames) of a workgroup of the info sweep
constexpr int kInfoLds = vc::kSelGramDoubles + 36 + 96 + 24 + 2 * 6 * vc::kSelMaxD + vc::kSelMaxCams * 256;      // doubles of LDS per wavefront there

struct SelView {
  SelRig rig;
  int n_frames, n_start, P;
  double prior;
  const double* poses;          // n_frames x kPoseStride
  const int* frame_view_off;    // n_frames + 1
  const int* view_cam;          // per view
  const int* view_off;          // per view + 1: into pt
  const int* pt;                // per corner: index of its target point
  const double* points;         // x 3
  const int* start;             // n_start frames
  double* info;                 // n_frames x P: packed I_f, unscaled
  int* fstat;                   // n_frames x 3: status, corners, behind
  double* scale;                // D
  double* S;                    // P: S_k, packed
  double* S_all;                // P
  double* piv;                  // D: pivots of S_k
  double* piv0;                 // D: pivots of S_0
  double* gains;                // n_frames: the last round that ran
  int* selected;                // n_frames: 1 = in the start set or picked
  int* state;                   // [0] picks so far, [1] stopped
  double* res;                  // [0] picks, [1] total, then per round: frame, gain, cum
};

template <int MODEL>
__device__ __forceinline__ void view_gram(const SelView& v, const vc::TileXf& x, const double* K, const vc::ModelPre& pre, int o0, int o1, int lane,
                                          double* G, int* corners, int* behind) {
  constexpr int NA = vc::sel_nacc(MODEL);
  double acc[NA];
#pragma unroll
  for (int a = 0; a < NA; ++a) acc[a] = 0.0;
  int ok = 0, bad = 0;
#pragma unroll 1
  for (int o = o0 + lane; o < o1; o += 64) {
    double r0[vc::kUCols], r1[vc::kUCols];
    const double* pw = v.points + 3 * (size_t)v.pt[o];
    const double p[3] = {pw[0], pw[1], pw[2]};
    if (vc::sel_corner_rows<MODEL>(x, K, pre, p, r0, r1)) { vc::sel_gram_add<MODEL>(r0, r1, acc); ++ok; } else ++bad;
  }
#pragma unroll
  for (int a = 0; a < NA; ++a) acc[a] = vc::wave_allsum(acc[a]);
  *corners = vc::wave_allsum(ok);
  *behind = vc::wave_allsum(bad);
  if (lane == 0) vc::sel_gram_expand<MODEL>(acc, G);
}

__global__ __launch_bounds__(64 * kInfoWaves) void k_select_info(SelView v) {
  __shared__ double s_all[kInfoWaves][kInfoLds];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int f = blockIdx.x * kInfoWaves + wave;
  if (f >= v.n_frames) return;                                    // (wave-uniform; no workgroup barrier below)
  double* G = s_all[wave];
  double* Hff = G + vc::kSelGramDoubles;
  double* W16 = Hff + 36;
  double* tmp = W16 + 96;
  double* Wf = tmp + 24;                                          // 6 x kSelMaxD
  double* Y = Wf + 6 * vc::kSelMaxD;                              // 6 x kSelMaxD
  double* Hcc = Y + 6 * vc::kSelMaxD;                             // per camera 16 x 16
  const SelRig& rig = v.rig;
  const int D = rig.D;
  for (int k = lane; k < 6 * vc::kSelMaxD; k += 64) Wf[k] = 0.0;
  if (lane < 36) Hff[lane] = 0.0;
  if (lane < 24) tmp[lane] = 0.0;
  vc::wave_lds_sync_local();
  unsigned seen = 0;
  int corners = 0, behind = 0;
  const double* T_wk = v.poses + (size_t)f * vc::kPoseStride;
  for (int t = v.frame_view_off[f]; t < v.frame_view_off[f + 1]; ++t) {
    const int c = v.view_cam[t];
    const double* cam = rig.cam + c * vc::kCamStride;
    vc::TileXf x;
    double K[10];
    vc::view_setup(T_wk, cam, &x, K);
    vc::ModelPre pre;
    vc::model_precompute(rig.model[c], K, &pre);
    int n_ok = 0, n_bad = 0;
    vc::with_model(rig.model[c], [&](auto m) { view_gram<decltype(m)::value>(v, x, K, pre, v.view_off[t], v.view_off[t + 1], lane, G, &n_ok, &n_bad); });
    corners += n_ok; behind += n_bad;
    if (n_ok == 0) { vc::wave_lds_sync_local(); continue; }
    vc::wave_lds_sync_local();
    if (lane == 0) vc::sel_view_blocks(G, cam, rig.model[c], rig.flags[c], Hff, W16, Hcc + c * 256, tmp);
    vc::wave_lds_sync_local();
    if (lane < rig.ncols[c])
      for (int r = 0; r < 6; ++r) Wf[r * vc::kSelMaxD + rig.col0[c] + lane] = W16[r * vc::kUCols + lane];
    seen |= 1u << c;
    vc::wave_lds_sync_local();
  }
  double L[36], dinv[6];
#pragma unroll
  for (int k = 0; k < 36; ++k) L[k] = Hff[k];
  const bool chol_ok = corners >= 4 && vc::sel_chol6(L, dinv);
  const int status = vc::sel_frame_status(corners, behind, chol_ok);
  if (lane == 0) { v.fstat[3 * f] = status; v.fstat[3 * f + 1] = corners; v.fstat[3 * f + 2] = behind; }
  double* out = v.info + (size_t)f * v.P;
  if (!vc::sel_usable(status)) {
    for (int e = lane; e < v.P; e += 64) out[e] = 0.0;
    return;
  }
  if (lane < D) vc::sel_schur_col(L, dinv, Wf, vc::kSelMaxD, lane, Y + lane, vc::kSelMaxD);
  vc::wave_lds_sync_local();
  for (int i = 0; i < D; ++i) {
    const int j = i + lane;
    if (j >= D) continue;
    const int ci = vc::sel_col_cam(rig, i), cj = vc::sel_col_cam(rig, j);
    const double hss = (ci == cj && ((seen >> ci) & 1u)) ? Hcc[ci * 256 + (i - rig.col0[ci]) * vc::kUCols + (j - rig.col0[ci])] : 0.0;
    out[vc::sel_pack_idx(i, j, D)] = vc::sel_info_entry(hss, Y, vc::kSelMaxD, i, j);
  }
}

__global__ __launch_bounds__(64) void k_select_scale(SelView v) {
  const int j = threadIdx.x;
  if (j >= v.rig.D) return;
  const int e = vc::sel_pack_idx(j, j, v.rig.D);
  double t = 0.0;
  for (int f = 0; f < v.n_frames; ++f)
    if (vc::sel_usable(v.fstat[3 * f])) t += v.info[(size_t)f * v.P + e];
  v.scale[j] = vc::sel_scale(t);
}

// packed entry e -> (i, j), i <= j
__device__ __forceinline__ void unpack_idx(int e, int D, int* i, int* j) {
  int r = 0;
  while (e >= D - r) { e -= D - r; ++r; }
  *i = r; *j = r + e;
}

__global__ __launch_bounds__(256) void k_select_init(SelView v) {
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e == 0) { v.state[0] = 0; v.state[1] = 0; }
  if (e >= v.P) return;
  int i, j;
  unpack_idx(e, v.rig.D, &i, &j);
  const double si = v.scale[i], sj = v.scale[j];
  double s0 = i == j ? v.prior : 0.0;
  for (int k = 0; k < v.n_start; ++k) s0 += vc::sel_scaled(v.info[(size_t)v.start[k] * v.P + e], si, sj);
  double sa = s0;
  for (int f = 0; f < v.n_frames; ++f)
    if (!v.selected[f] && vc::sel_usable(v.fstat[3 * f])) sa += vc::sel_scaled(v.info[(size_t)f * v.P + e], si, sj);
  v.S[e] = s0; v.S_all[e] = sa;
}

// packed S (+ scaled I_f when info != nullptr) expanded into the upper triangle of M (LDS, ld D) and factored: the wave's lanes are columns
__device__ __forceinline__ void wave_expand_factor(double* M, const double* S, const double* info, const double* scale, int D, int lane) {
  const double sj = (info && lane < D) ? scale[lane] : 0.0;
  for (int i = 0; i <= lane && lane < D; ++i) {
    const int e = vc::sel_pack_idx(i, lane, D);
    M[i * D + lane] = info ? S[e] + vc::sel_scaled(info[e], scale[i], sj) : S[e];
  }
  vc::wave_lds_sync_local();
  for (int k = 0; k + 1 < D; ++k) {
    if (lane > k && lane < D) vc::sel_chol_step(M, D, k, lane);
    vc::wave_lds_sync_local();
  }
}
// sum over the pivots of log(p'_k / p_k) in every lane; -1 where a pivot is not positive
__device__ __forceinline__ double wave_pivot_gain(const double* M, const double* piv, int D, int lane) {
  const double p = lane < D ? M[lane * D + lane] : 1.0, q = lane < D ? piv[lane] : 1.0;
  const bool ok = p > 0.0 && q > 0.0;
  const double g = vc::wave_allsum(ok ? vc::sel_gain_term(p, q) : 0.0);
  return vc::wave_allsum(ok ? 0 : 1) == 0 ? g : -1.0;
}

__global__ __launch_bounds__(64) void k_select_logdet0(SelView v) {
  extern __shared__ __attribute__((aligned(16))) double s_m[];
  const int lane = threadIdx.x, D = v.rig.D;
  wave_expand_factor(s_m, v.S, nullptr, nullptr, D, lane);
  if (lane < D) { const double p = s_m[lane * D + lane]; v.piv0[lane] = p; v.piv[lane] = p; }
  vc::wave_lds_sync_local();
  wave_expand_factor(s_m, v.S_all, nullptr, nullptr, D, lane);
  const double total = wave_pivot_gain(s_m, v.piv0, D, lane);
  if (lane == 0) { v.res[0] = 0.0; v.res[1] = total; }
}

__global__ __launch_bounds__(256) void k_select_gain(SelView v, double* gains, int force) {
  extern __shared__ __attribute__((aligned(16))) double s_m[];
  if (!force && v.state[1]) return;                               // a round after the stop does nothing
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, D = v.rig.D;
  const int f = blockIdx.x * (blockDim.x >> 6) + wave;
  if (f >= v.n_frames) return;
  if (v.selected[f] || !vc::sel_usable(v.fstat[3 * f])) { if (lane == 0) gains[f] = -1.0; return; }
  double* M = s_m + (size_t)wave * D * D;
  wave_expand_factor(M, v.S, v.info + (size_t)f * v.P, v.scale, D, lane);
  const double g = wave_pivot_gain(M, v.piv, D, lane);
  if (lane == 0) gains[f] = g;
}

__global__ __launch_bounds__(64) void k_select_pick(SelView v, int dry) {
  extern __shared__ __attribute__((aligned(16))) double s_m[];
  if (!dry && v.state[1]) return;
  const int lane = threadIdx.x, D = v.rig.D;
  double best = -1.0;
  int idx = -1;
  for (int f = lane; f < v.n_frames; f += 64) {                   // (ascending frames within a lane)
    const double g = v.gains[f];
    if (g >= 0.0 && vc::sel_better(g, f, best, idx)) { best = g; idx = f; }
  }
  vc::wave_argmax_low(&best, &idx);
  if (idx < 0 || !(best > 0.0)) { if (lane == 0 && !dry) v.state[1] = 1; return; }
  const double* info = v.info + (size_t)idx * v.P;
  wave_expand_factor(s_m, v.S, info, v.scale, D, lane);
  const double cum = wave_pivot_gain(s_m, v.piv0, D, lane);
  if (dry) return;
  const double sj = lane < D ? v.scale[lane] : 0.0;
  for (int i = 0; i <= lane && lane < D; ++i) {
    const int e = vc::sel_pack_idx(i, lane, D);
    v.S[e] = v.S[e] + vc::sel_scaled(info[e], v.scale[i], sj);
  }
  if (lane < D) v.piv[lane] = s_m[lane * D + lane];
  if (lane == 0) {
    const int k = v.state[0];
    double* r = v.res + 2 + 3 * (size_t)k;
    r[0] = (double)idx; r[1] = best; r[2] = cum;
    v.state[0] = k + 1; v.res[0] = (double)(k + 1);
    v.selected[idx] = 1;
  }
}

__global__ __launch_bounds__(256) void k_select_mark(SelView v) {
  const int k = blockIdx.x * 256 + threadIdx.x;
  if (k < v.n_start) v.selected[v.start[k]] = 1;
}

}  // namespace

struct vc_selector {
  int device = 0;
  hipStream_t stream = nullptr;
  SelRig rig;
  // ---- input (host) ----
  std::vector<int> o_frame, o_cam, o_pt;         // corners in the order of arrival
  std::vector<double> points;                     // x 3
  std::vector<double> poses;                      // n x 7
  int n_named = 0;                                // 1 + the largest frame a tile has named
  bool input_dirty = true;
  // ---- device ----
  unsigned char* d_buf = nullptr;
  SelView v;
  double* d_gains_tmp = nullptr;                  // the timer's gains
  bool have_info = false, have_run = false;
  int rounds = 0;
  // ---- results ----
  std::vector<int> fstat;
  std::vector<double> res, scale;
  int n_frames() const { return (int)(poses.size() / 7); }
  int gain_waves() const { const int w = (int)(65536 / ((size_t)rig.D * rig.D * 8)); return w < 1 ? 1 : (w > 4 ? 4 : w); }
};

namespace {

bool stream_ok(vc_selector* s) { return hipGetLastError() == hipSuccess && hipStreamSynchronize(s->stream) == hipSuccess; }

void launch_info(vc_selector* s) {
  hipLaunchKernelGGL(k_select_info, dim3((s->v.n_frames + kInfoWaves - 1) / kInfoWaves), dim3(64 * kInfoWaves), 0, s->stream, s->v);
}
void launch_gain(vc_selector* s, double* gains, int force) {
  const int w = s->gain_waves(), D = s->rig.D;
  hipLaunchKernelGGL(k_select_gain, dim3((s->v.n_frames + w - 1) / w), dim3(64 * w), (size_t)w * D * D * 8, s->stream, s->v, gains, force);
}
void launch_pick(vc_selector* s, int dry) {
  const int D = s->rig.D;
  hipLaunchKernelGGL(k_select_pick, dim3(1), dim3(64), (size_t)D * D * 8, s->stream, s->v, dry);
}

// the device image of the input: views ordered by frame, then camera; the corners of a view in the order of arrival
int upload_input(vc_selector* s) {
  const int N = s->n_frames(), D = s->rig.D, P = vc::sel_pack_len(D);
  const size_t M = s->o_frame.size();
  std::vector<size_t> ord(M);
  std::iota(ord.begin(), ord.end(), (size_t)0);
  std::stable_sort(ord.begin(), ord.end(), [&](size_t a, size_t b) {
    return s->o_frame[a] != s->o_frame[b] ? s->o_frame[a] < s->o_frame[b] : s->o_cam[a] < s->o_cam[b];
  });
  std::vector<int> frame_view_off(N + 1, 0), view_cam, view_off, pt(M);
  {
    size_t k = 0;
    for (int f = 0; f < N; ++f) {
      frame_view_off[f] = (int)view_cam.size();
      while (k < M && s->o_frame[ord[k]] == f) {
        const int c = s->o_cam[ord[k]];
        view_cam.push_back(c); view_off.push_back((int)k);
        while (k < M && s->o_frame[ord[k]] == f && s->o_cam[ord[k]] == c) { pt[k] = s->o_pt[ord[k]]; ++k; }
      }
    }
    frame_view_off[N] = (int)view_cam.size();
    view_off.push_back((int)M);
  }
  std::vector<double> poses((size_t)N * vc::kPoseStride, 0.0);
  for (int f = 0; f < N; ++f) std::memcpy(&poses[(size_t)f * vc::kPoseStride], &s->poses[(size_t)f * 7], 56);
  if (s->d_buf) { (void)hipStreamSynchronize(s->stream); (void)hipFree(s->d_buf); s->d_buf = nullptr; }
  SelView& v = s->v;
  double* d_poses = nullptr; int *d_fvo = nullptr, *d_vc = nullptr, *d_vo = nullptr, *d_pt = nullptr, *d_start = nullptr; double* d_points = nullptr;
  auto carve = [&](vch::Carver q) {
    d_poses = q.take<double>(poses.size());
    d_fvo = q.take<int>(frame_view_off.size()); d_vc = q.take<int>(view_cam.size() + 1); d_vo = q.take<int>(view_off.size()); d_pt = q.take<int>(M + 1);
    d_points = q.take<double>(s->points.size() + 3);
    d_start = q.take<int>((size_t)N);
    v.info = q.take<double>((size_t)N * P);
    v.fstat = q.take<int>((size_t)N * 3);
    v.scale = q.take<double>(D); v.S = q.take<double>(P); v.S_all = q.take<double>(P); v.piv = q.take<double>(D); v.piv0 = q.take<double>(D);
    v.gains = q.take<double>((size_t)N); s->d_gains_tmp = q.take<double>((size_t)N);
    v.selected = q.take<int>((size_t)N); v.state = q.take<int>(2);
    v.res = q.take<double>(2 + 3 * (size_t)N);
    return q.bytes();
  };
  if (hipMalloc((void**)&s->d_buf, carve(vch::Carver())) != hipSuccess) { s->d_buf = nullptr; return VC_ERR_NO_DEVICE; }
  carve(vch::Carver(s->d_buf));
  v.rig = s->rig; v.n_frames = N; v.P = P; v.n_start = 0; v.prior = 0.0;
  v.poses = d_poses; v.frame_view_off = d_fvo; v.view_cam = d_vc; v.view_off = d_vo; v.pt = d_pt; v.points = d_points; v.start = d_start;
  auto up = [&](void* dst, const void* src, size_t bytes) { return bytes == 0 || hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, s->stream) == hipSuccess; };
  if (!up(d_poses, poses.data(), poses.size() * 8) || !up(d_fvo, frame_view_off.data(), frame_view_off.size() * 4) ||
      !up(d_vc, view_cam.data(), view_cam.size() * 4) || !up(d_vo, view_off.data(), view_off.size() * 4) || !up(d_pt, pt.data(), M * 4) ||
      !up(d_points, s->points.data(), s->points.size() * 8) || hipStreamSynchronize(s->stream) != hipSuccess) return VC_ERR_NO_DEVICE;
  return VC_OK;
}

// the info sweep and the scale, once per input
int ensure_info(vc_selector* s) {
  if (s->have_info && !s->input_dirty) return VC_OK;
  s->have_info = false;
  const int rc = upload_input(s);
  if (rc != VC_OK) return rc;
  const int N = s->v.n_frames, D = s->rig.D;
  launch_info(s);
  hipLaunchKernelGGL(k_select_scale, dim3(1), dim3(64), 0, s->stream, s->v);
  s->fstat.assign((size_t)N * 3, 0); s->scale.assign(D, 1.0);
  if (hipGetLastError() != hipSuccess || hipMemcpyAsync(s->fstat.data(), s->v.fstat, (size_t)N * 12, hipMemcpyDeviceToHost, s->stream) != hipSuccess ||
      hipMemcpyAsync(s->scale.data(), s->v.scale, (size_t)D * 8, hipMemcpyDeviceToHost, s->stream) != hipSuccess || !stream_ok(s)) return VC_ERR_NO_DEVICE;
  s->input_dirty = false; s->have_info = true;
  return VC_OK;
}

}  // namespace

extern "C" {

int vc_selector_create(int device, int n_cameras, const int* model, const double* params, const int* nparams, const double* T_ck, const int* cam_flags,
                       vc_selector** out) {
  if (!out || n_cameras < 1 || n_cameras > vc::kSelMaxCams || !model || !params || !nparams || !T_ck || !cam_flags) return VC_ERR_BAD_ARG;
  SelRig rig;
  std::memset(&rig, 0, sizeof(rig));
  rig.n_cams = n_cameras;
  for (int c = 0; c < n_cameras; ++c) {
    const int nk = vc::model_nk(model[c]);
    if (nk < 0 || nparams[c] != nk || (cam_flags[c] & ~7) != 0) return VC_ERR_BAD_ARG;
    for (int k = 0; k < nk; ++k) if (!std::isfinite(params[10 * c + k])) return VC_ERR_BAD_ARG;
    for (int k = 0; k < 7; ++k) if (!std::isfinite(T_ck[7 * c + k])) return VC_ERR_BAD_ARG;
    rig.model[c] = model[c]; rig.flags[c] = cam_flags[c];
    std::memcpy(rig.cam + c * vc::kCamStride, T_ck + 7 * c, 56);
    std::memcpy(rig.cam + c * vc::kCamStride + vc::kCamK, params + 10 * c, (size_t)nk * 8);
  }
  if (!vc::sel_layout(&rig)) return VC_ERR_UNSUPPORTED;
  if (rig.D < 1) return VC_ERR_BAD_ARG;
  if (vch::open_device(device) != VC_OK) return VC_ERR_NO_DEVICE;
  vc_selector* s = new vc_selector;
  s->device = device; s->rig = rig;
  std::memset(&s->v, 0, sizeof(s->v));
  if (hipStreamCreate(&s->stream) != hipSuccess) { s->stream = nullptr; vc_selector_destroy(s); return VC_ERR_NO_DEVICE; }
  *out = s;
  return VC_OK;
}
void vc_selector_destroy(vc_selector* s) {
  if (!s) return;
  (void)hipSetDevice(s->device);
  if (s->stream) { (void)hipStreamSynchronize(s->stream); (void)hipStreamDestroy(s->stream); }
  (void)hipFree(s->d_buf);
  delete s;
}

int vc_select_add_tiles(vc_selector* s, int n_tiles, const int* tile_frame, const int* tile_cam, const long long* tile_off, const double* points, int n_points,
                        const int* point_id) {
  if (!s || n_tiles < 0 || n_points < 0 || (n_tiles > 0 && (!tile_frame || !tile_cam || !tile_off))) return VC_ERR_BAD_ARG;
  if (n_tiles == 0) return VC_OK;
  if (tile_off[0] < 0) return VC_ERR_BAD_ARG;
  int named = s->n_named;
  for (int t = 0; t < n_tiles; ++t) {
    if (tile_frame[t] < 0 || tile_cam[t] < 0 || tile_cam[t] >= s->rig.n_cams || tile_off[t + 1] < tile_off[t]) return VC_ERR_BAD_ARG;
    named = std::max(named, tile_frame[t] + 1);
  }
  const long long m = tile_off[n_tiles];
  if (m > tile_off[0] && (!points || !point_id)) return VC_ERR_BAD_ARG;
  for (long long o = tile_off[0]; o < m; ++o) if (point_id[o] < 0 || point_id[o] >= n_points) return VC_ERR_BAD_ARG;
  for (int k = 0; k < 3 * n_points; ++k) if (!std::isfinite(points[k])) return VC_ERR_BAD_ARG;
  const int base = (int)(s->points.size() / 3);
  s->points.insert(s->points.end(), points, points + 3 * (size_t)n_points);
  for (int t = 0; t < n_tiles; ++t)
    for (long long o = tile_off[t]; o < tile_off[t + 1]; ++o) { s->o_frame.push_back(tile_frame[t]); s->o_cam.push_back(tile_cam[t]); s->o_pt.push_back(base + point_id[o]); }
  s->n_named = named;
  s->input_dirty = true; s->have_run = false;
  return VC_OK;
}

int vc_select_set_poses(vc_selector* s, const double* T_wk, int n_frames) {
  if (!s || !T_wk || n_frames < 1) return VC_ERR_BAD_ARG;
  for (int k = 0; k < 7 * n_frames; ++k) if (!std::isfinite(T_wk[k])) return VC_ERR_BAD_ARG;
  s->poses.assign(T_wk, T_wk + 7 * (size_t)n_frames);
  s->input_dirty = true; s->have_run = false;
  return VC_OK;
}

int vc_select_run(vc_selector* s, int k, const int* start_set, int n_start, double prior) {
  if (!s || k < 1 || n_start < 0 || (n_start > 0 && !start_set) || !vc::sel_prior_ok(prior)) return VC_ERR_BAD_ARG;
  const int N = s->n_frames();
  if (N < 1 || s->n_named > N) return VC_ERR_BAD_ARG;             // poses missing
  {
    std::vector<char> in(N, 0);
    for (int i = 0; i < n_start; ++i) {
      if (start_set[i] < 0 || start_set[i] >= N || in[start_set[i]]) return VC_ERR_BAD_ARG;
      in[start_set[i]] = 1;
    }
  }
  s->have_run = false;
  if (hipSetDevice(s->device) != hipSuccess) return VC_ERR_NO_DEVICE;
  int rc = ensure_info(s);
  if (rc != VC_OK) return rc;
  SelView& v = s->v;
  const int D = s->rig.D;
  v.n_start = n_start; v.prior = prior;
  if ((n_start > 0 && hipMemcpyAsync((void*)v.start, start_set, (size_t)n_start * 4, hipMemcpyHostToDevice, s->stream) != hipSuccess) ||
      hipMemsetAsync(v.selected, 0, (size_t)N * 4, s->stream) != hipSuccess || hipMemsetAsync(v.res, 0, (2 + 3 * (size_t)N) * 8, s->stream) != hipSuccess)
    return VC_ERR_NO_DEVICE;
  if (n_start > 0) hipLaunchKernelGGL(k_select_mark, dim3((n_start + 255) / 256), dim3(256), 0, s->stream, v);
  hipLaunchKernelGGL(k_select_init, dim3((v.P + 255) / 256), dim3(256), 0, s->stream, v);
  hipLaunchKernelGGL(k_select_logdet0, dim3(1), dim3(64), (size_t)D * D * 8, s->stream, v);
  s->rounds = std::min(k, N);
  for (int r = 0; r < s->rounds; ++r) { launch_gain(s, v.gains, 0); launch_pick(s, 0); }
  s->res.assign(2 + 3 * (size_t)N, 0.0);
  if (hipGetLastError() != hipSuccess || hipMemcpyAsync(s->res.data(), v.res, s->res.size() * 8, hipMemcpyDeviceToHost, s->stream) != hipSuccess || !stream_ok(s))
    return VC_ERR_NO_DEVICE;
  s->have_run = true;
  return VC_OK;
}

int vc_select_get(vc_selector* s, int* n_picked, int* order, double* gain, double* cum, double* total) {
  if (!s || !s->have_run) return VC_ERR_BAD_ARG;
  const int n = (int)s->res[0];
  if (n_picked) *n_picked = n;
  if (total) *total = s->res[1];
  for (int k = 0; k < n; ++k) {
    const double* r = &s->res[2 + 3 * (size_t)k];
    if (order) order[k] = (int)r[0];
    if (gain) gain[k] = r[1];
    if (cum) cum[k] = r[2];
  }
  return VC_OK;
}

int vc_select_frames(vc_selector* s, int* status, int* corners, int* behind) {
  if (!s || !s->have_run) return VC_ERR_BAD_ARG;
  for (int f = 0; f < s->n_frames(); ++f) {
    if (status) status[f] = s->fstat[3 * (size_t)f];
    if (corners) corners[f] = s->fstat[3 * (size_t)f + 1];
    if (behind) behind[f] = s->fstat[3 * (size_t)f + 2];
  }
  return VC_OK;
}

int vc_select_frame_information(vc_selector* s, int frame, double* I, double* scale) {
  if (!s || !s->have_run || frame < 0 || frame >= s->n_frames()) return VC_ERR_BAD_ARG;
  const int D = s->rig.D, P = s->v.P;
  if (scale) std::memcpy(scale, s->scale.data(), (size_t)D * 8);
  if (!I) return VC_OK;
  std::vector<double> packed(P);
  if (hipSetDevice(s->device) != hipSuccess || hipMemcpy(packed.data(), s->v.info + (size_t)frame * P, (size_t)P * 8, hipMemcpyDeviceToHost) != hipSuccess)
    return VC_ERR_NO_DEVICE;
  for (int i = 0; i < D; ++i)
    for (int j = i; j < D; ++j) { I[i * D + j] = packed[vc::sel_pack_idx(i, j, D)]; I[j * D + i] = I[i * D + j]; }
  return VC_OK;
}

int vc_select_last_gains(vc_selector* s, double* gains) {
  if (!s || !s->have_run || !gains) return VC_ERR_BAD_ARG;
  if (hipSetDevice(s->device) != hipSuccess || hipMemcpy(gains, s->v.gains, (size_t)s->n_frames() * 8, hipMemcpyDeviceToHost) != hipSuccess) return VC_ERR_NO_DEVICE;
  return VC_OK;
}

int vc_select_dim(vc_selector* s) { return s ? s->rig.D : VC_ERR_BAD_ARG; }

int vc_time_select(vc_selector* s, int reps, double out_ms[3]) {
  if (!s || reps < 1 || !out_ms || !s->have_run) return VC_ERR_BAD_ARG;
  if (hipSetDevice(s->device) != hipSuccess) return VC_ERR_NO_DEVICE;
  for (int what = 0; what < 3; ++what) {
    auto launch = [&]() {                                          // (the info sweep rewrites the same bits; the gain round writes the timer's own array; the pick stores nothing)
      if (what == 0) launch_info(s);
      else if (what == 1) launch_gain(s, s->d_gains_tmp, 1);
      else launch_pick(s, 1);
    };
    const int rc = vch::time_back_to_back(s->stream, reps, launch, &out_ms[what]);
    if (rc != VC_OK) return rc;
  }
  return VC_OK;
}

}  // extern "C"
