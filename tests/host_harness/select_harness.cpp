// TEST INFRASTRUCTURE: the arithmetic of view selection (vicalib_amd/csrc/vc_select.hpp, VC_HD) compiled for the host, so that the CPU suite can
// hold the frame information, the scaling, the gains and the pick rule against numpy without a GPU.  The rows of a corner, the view blocks, the
// 6 x 6 factorisation, the Schur complement, the packed layout, the factorisation step, the gain term and the pick rule are the very functions
// the kernels run; what the kernels add is the indexing and the order of the sums over corners, which are plain loops in corner order here.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <numeric>
#include <thread>
#include <vector>
#include "../../vicalib_amd/csrc/vc_select.hpp"

namespace {

template <class F>
void parallel_for(int n, int threads, F&& body) {
  if (threads <= 1 || n < 2) { for (int i = 0; i < n; ++i) body(i); return; }
  std::vector<std::thread> pool;
  for (int t = 0; t < threads; ++t) pool.emplace_back([&, t]() { for (int i = t; i < n; i += threads) body(i); });
  for (auto& th : pool) th.join();
}

template <int MODEL>
void view_gram(const vc::TileXf& x, const double* K, const vc::ModelPre& pre, const double* points, const int* pt, int n, double* G, int* corners, int* behind) {
  double acc[vc::sel_nacc(MODEL)];
  for (double& a : acc) a = 0.0;
  for (int o = 0; o < n; ++o) {
    double r0[vc::kUCols], r1[vc::kUCols];
    if (vc::sel_corner_rows<MODEL>(x, K, pre, points + 3 * (size_t)pt[o], r0, r1)) { vc::sel_gram_add<MODEL>(r0, r1, acc); ++*corners; } else ++*behind;
  }
  vc::sel_gram_expand<MODEL>(acc, G);
}

// S (+ scaled packed info) expanded and factored; the pivots on the diagonal of M
void expand_factor(std::vector<double>& M, const double* S, const double* info, const double* scale, int D) {
  for (int j = 0; j < D; ++j)
    for (int i = 0; i <= j; ++i) {
      const int e = vc::sel_pack_idx(i, j, D);
      M[i * D + j] = info ? S[e] + vc::sel_scaled(info[e], scale[i], scale[j]) : S[e];
    }
  for (int k = 0; k + 1 < D; ++k)
    for (int j = k + 1; j < D; ++j) vc::sel_chol_step(M.data(), D, k, j);
}
double pivot_gain(const std::vector<double>& M, const double* piv, int D) {
  double g = 0.0;
  for (int k = 0; k < D; ++k) {
    if (!(M[k * D + k] > 0.0) || !(piv[k] > 0.0)) return -1.0;
    g += vc::sel_gain_term(M[k * D + k], piv[k]);
  }
  return g;
}

}  // namespace

extern "C" {

// One whole selection.  info = n_frames x D x D (unscaled); fstat = n_frames x [status, corners, behind]; order / gain / cum: n_frames each;
// last_gains: n_frames.  Returns 0, -2 (VC_ERR_BAD_ARG) or -7 (VC_ERR_UNSUPPORTED: D > 64, *D_out still set).
int vch_select(int n_cams, const int* model, const double* params, const double* T_ck, const int* flags, int n_frames, const double* T_wk, int n_tiles,
               const int* tile_frame, const int* tile_cam, const long long* tile_off, const double* points, const int* point_id, int k, const int* start, int n_start,
               double prior, int threads, int* D_out, int* fstat, double* info, double* scale, int* n_picked, int* order, double* gain, double* cum, double* total,
               double* last_gains) {
  if (n_cams < 1 || n_cams > vc::kSelMaxCams || n_frames < 1 || k < 1 || !vc::sel_prior_ok(prior)) return -2;
  vc::SelRig rig;
  std::memset(&rig, 0, sizeof(rig));
  rig.n_cams = n_cams;
  for (int c = 0; c < n_cams; ++c) {
    const int nk = vc::model_nk(model[c]);
    if (nk < 0) return -2;
    rig.model[c] = model[c]; rig.flags[c] = flags[c];
    std::memcpy(rig.cam + c * vc::kCamStride, T_ck + 7 * c, 56);
    std::memcpy(rig.cam + c * vc::kCamStride + vc::kCamK, params + 10 * c, (size_t)nk * 8);
  }
  const bool fits = vc::sel_layout(&rig);
  *D_out = rig.D;
  if (!fits) return -7;
  const int D = rig.D, P = vc::sel_pack_len(D), N = n_frames;
  // the views of every frame ordered by camera, a view's corners in the order of arrival
  std::vector<int> o_frame, o_cam, o_pt;
  for (int t = 0; t < n_tiles; ++t)
    for (long long o = tile_off[t]; o < tile_off[t + 1]; ++o) { o_frame.push_back(tile_frame[t]); o_cam.push_back(tile_cam[t]); o_pt.push_back(point_id[o]); }
  const size_t M = o_frame.size();
  std::vector<size_t> ord(M);
  std::iota(ord.begin(), ord.end(), (size_t)0);
  std::stable_sort(ord.begin(), ord.end(), [&](size_t a, size_t b) { return o_frame[a] != o_frame[b] ? o_frame[a] < o_frame[b] : o_cam[a] < o_cam[b]; });
  std::vector<int> frame_first(N + 1, 0), pt(M);
  {
    size_t q = 0;
    for (int f = 0; f < N; ++f) { frame_first[f] = (int)q; while (q < M && o_frame[ord[q]] == f) { pt[q] = o_pt[ord[q]]; ++q; } }
    frame_first[N] = (int)q;
    if (q != M) return -2;                                          // a tile names a frame without a pose
  }
  std::vector<double> packed((size_t)N * P, 0.0);
  parallel_for(N, threads, [&](int f) {
    std::vector<double> G(vc::kSelGramDoubles), Hcc((size_t)vc::kSelMaxCams * 256, 0.0), Wf(6 * vc::kSelMaxD, 0.0), Y(6 * vc::kSelMaxD, 0.0);
    double Hff[36] = {0}, W16[96], tmp[24] = {0};
    unsigned seen = 0;
    int corners = 0, behind = 0;
    int q = frame_first[f];
    while (q < frame_first[f + 1]) {
      const int c = o_cam[ord[q]];
      int q1 = q;
      while (q1 < frame_first[f + 1] && o_cam[ord[q1]] == c) ++q1;
      const double* cam = rig.cam + c * vc::kCamStride;
      vc::TileXf x;
      double K[10];
      vc::view_setup(T_wk + 7 * (size_t)f, cam, &x, K);
      vc::ModelPre pre;
      vc::model_precompute(rig.model[c], K, &pre);
      int n_ok = 0, n_bad = 0;
      vc::with_model(rig.model[c], [&](auto m) { view_gram<decltype(m)::value>(x, K, pre, points, &pt[q], q1 - q, G.data(), &n_ok, &n_bad); });
      corners += n_ok; behind += n_bad;
      if (n_ok > 0) {
        vc::sel_view_blocks(G.data(), cam, rig.model[c], rig.flags[c], Hff, W16, &Hcc[(size_t)c * 256], tmp);
        for (int j = 0; j < rig.ncols[c]; ++j)
          for (int r = 0; r < 6; ++r) Wf[r * vc::kSelMaxD + rig.col0[c] + j] = W16[r * vc::kUCols + j];
        seen |= 1u << c;
      }
      q = q1;
    }
    double dinv[6];
    const bool chol_ok = corners >= 4 && vc::sel_chol6(Hff, dinv);
    const int status = vc::sel_frame_status(corners, behind, chol_ok);
    fstat[3 * f] = status; fstat[3 * f + 1] = corners; fstat[3 * f + 2] = behind;
    if (!vc::sel_usable(status)) return;
    for (int j = 0; j < D; ++j) vc::sel_schur_col(Hff, dinv, Wf.data(), vc::kSelMaxD, j, &Y[j], vc::kSelMaxD);
    for (int i = 0; i < D; ++i)
      for (int j = i; j < D; ++j) {
        const int ci = vc::sel_col_cam(rig, i), cj = vc::sel_col_cam(rig, j);
        const double hss = (ci == cj && ((seen >> ci) & 1u)) ? Hcc[(size_t)ci * 256 + (i - rig.col0[ci]) * vc::kUCols + (j - rig.col0[ci])] : 0.0;
        packed[(size_t)f * P + vc::sel_pack_idx(i, j, D)] = vc::sel_info_entry(hss, Y.data(), vc::kSelMaxD, i, j);
      }
  });
  for (int f = 0; f < N; ++f)
    for (int i = 0; i < D; ++i)
      for (int j = i; j < D; ++j) { const double x = packed[(size_t)f * P + vc::sel_pack_idx(i, j, D)]; info[((size_t)f * D + i) * D + j] = x; info[((size_t)f * D + j) * D + i] = x; }
  for (int j = 0; j < D; ++j) {
    double t = 0.0;
    for (int f = 0; f < N; ++f) if (vc::sel_usable(fstat[3 * f])) t += packed[(size_t)f * P + vc::sel_pack_idx(j, j, D)];
    scale[j] = vc::sel_scale(t);
  }
  std::vector<char> selected(N, 0);
  for (int i = 0; i < n_start; ++i) { if (start[i] < 0 || start[i] >= N || selected[start[i]]) return -2; selected[start[i]] = 1; }
  std::vector<double> S(P), S_all(P), piv(D), piv0(D), Mx((size_t)D * D);
  for (int i = 0; i < D; ++i)
    for (int j = i; j < D; ++j) {
      const int e = vc::sel_pack_idx(i, j, D);
      double s0 = i == j ? prior : 0.0;
      for (int q = 0; q < n_start; ++q) s0 += vc::sel_scaled(packed[(size_t)start[q] * P + e], scale[i], scale[j]);
      double sa = s0;
      for (int f = 0; f < N; ++f) if (!selected[f] && vc::sel_usable(fstat[3 * f])) sa += vc::sel_scaled(packed[(size_t)f * P + e], scale[i], scale[j]);
      S[e] = s0; S_all[e] = sa;
    }
  expand_factor(Mx, S.data(), nullptr, nullptr, D);
  for (int q = 0; q < D; ++q) { piv0[q] = Mx[q * D + q]; piv[q] = piv0[q]; }
  expand_factor(Mx, S_all.data(), nullptr, nullptr, D);
  *total = pivot_gain(Mx, piv0.data(), D);
  *n_picked = 0;
  for (int f = 0; f < N; ++f) last_gains[f] = 0.0;
  const int rounds = std::min(k, N);
  for (int r = 0; r < rounds; ++r) {
    parallel_for(N, threads, [&](int f) {
      if (selected[f] || !vc::sel_usable(fstat[3 * f])) { last_gains[f] = -1.0; return; }
      std::vector<double> Mf((size_t)D * D);
      expand_factor(Mf, S.data(), &packed[(size_t)f * P], scale, D);
      last_gains[f] = pivot_gain(Mf, piv.data(), D);
    });
    double best = -1.0;
    int idx = -1;
    for (int f = 0; f < N; ++f) if (last_gains[f] >= 0.0 && vc::sel_better(last_gains[f], f, best, idx)) { best = last_gains[f]; idx = f; }
    if (idx < 0 || !(best > 0.0)) break;
    expand_factor(Mx, S.data(), &packed[(size_t)idx * P], scale, D);
    const double c = pivot_gain(Mx, piv0.data(), D);
    for (int i = 0; i < D; ++i)
      for (int j = i; j < D; ++j) { const int e = vc::sel_pack_idx(i, j, D); S[e] = S[e] + vc::sel_scaled(packed[(size_t)idx * P + e], scale[i], scale[j]); }
    for (int q = 0; q < D; ++q) piv[q] = Mx[q * D + q];
    order[*n_picked] = idx; gain[*n_picked] = best; cum[*n_picked] = c; ++*n_picked;
    selected[idx] = 1;
  }
  return 0;
}

}  // extern "C"
