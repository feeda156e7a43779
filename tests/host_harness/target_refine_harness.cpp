// TEST INFRASTRUCTURE: the arithmetic of the target step (vicalib_amd/csrc/vc_target_refine.hpp, VC_HD) compiled for the host, so that the CPU suite
// can hold it against numpy without a GPU.  The rows and the record of a corner, the view blocks, the 6 x 6 factorisation, the (frame, point)
// records, the pair blocks, the factorisation step of the shared columns, the gauge entries and the two thresholds are the very functions the
// kernels run; what the kernels add is the indexing, the order of the sums and the blocking of the dense factorisation, which are plain loops
// here (an unblocked Cholesky).  With -DTARGET_REFINE_HARNESS_MAIN the file is a program of its own on a small built-in case, for a sanitizer run.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <map>
#include <numeric>
#include <vector>
#include "../../vicalib_amd/csrc/vc_target_refine.hpp"

namespace {

template <int MODEL>
void view_sweep(const vc::TileXf& x, const double* K, const vc::ModelPre& pre, const double* Rck, int flags, const double* points, const int* pt, const double* z, int n,
                double* G, double* corner, int* corner_ok, int* corners, int* behind, double* cost) {
  double acc[vc::sel_nacc(MODEL)], accg[vc::sel_nu(MODEL)];
  for (double& a : acc) a = 0.0;
  for (double& a : accg) a = 0.0;
  for (int o = 0; o < n; ++o) {
    double r0[vc::kUCols], r1[vc::kUCols], r[2];
    double* out = corner + (size_t)o * vc::kTrCornerStride;
    if (vc::tr_corner_rows<MODEL>(x, K, pre, points + 3 * (size_t)pt[o], z + 2 * (size_t)o, r0, r1, r)) {
      vc::sel_gram_add<MODEL>(r0, r1, acc);
      vc::tr_grad_add<MODEL>(r0, r1, r[0], r[1], accg);
      vc::tr_corner_record<MODEL>(r0, r1, r, Rck, x.Rcw, flags, out);
      corner_ok[o] = 1; *cost += r[0] * r[0] + r[1] * r[1]; ++*corners;
    } else { vc::tr_corner_zero(out); corner_ok[o] = 0; ++*behind; }
  }
  vc::sel_gram_expand<MODEL>(acc, G);
  vc::tr_grad_place<MODEL>(accg, G);
}

}  // namespace

extern "C" {

// The arguments of vc_target_refine_batch without the device.  Returns 0, -2 (VC_ERR_BAD_ARG) or -7 (VC_ERR_UNSUPPORTED).
int vch_target_refine(int n_cams, const int* model, const double* params, const double* T_ck, const int* flags, int n_frames, const double* T_wk, int n_tiles,
                      const int* tile_frame, const int* tile_cam, const long long* tile_off, const int* point_id, const double* p_c, const double* points,
                      const double* nominal, int n_points, double lambda, double* refined, int* point_status, int* point_corners, int* frame_status, int* gauge_rank,
                      int* result_status, double* cost_out, double* pred_out) {
  if (n_cams < 1 || n_cams > vc::kSelMaxCams || n_frames < 1 || !vc::sel_prior_ok(lambda) || n_points < vc::kTrMinPoints) return -2;
  if (n_points > vc::kTrMaxPoints) return -7;
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
  if (!vc::sel_layout(&rig)) return -7;
  const int D = rig.D, N = n_frames, P = n_points, n = 3 * P;
  // corners ordered by frame, then camera, in the order of arrival
  std::vector<int> o_frame, o_cam, o_pt;
  std::vector<double> o_z;
  for (int t = 0; t < n_tiles; ++t) {
    if (tile_frame[t] < 0 || tile_frame[t] >= N || tile_cam[t] < 0 || tile_cam[t] >= n_cams) return -2;
    for (long long o = tile_off[t]; o < tile_off[t + 1]; ++o) {
      if (point_id[o] < 0 || point_id[o] >= P) return -2;
      o_frame.push_back(tile_frame[t]); o_cam.push_back(tile_cam[t]); o_pt.push_back(point_id[o]); o_z.push_back(p_c[2 * o]); o_z.push_back(p_c[2 * o + 1]);
    }
  }
  const size_t M = o_frame.size();
  std::vector<size_t> ord(M);
  std::iota(ord.begin(), ord.end(), (size_t)0);
  std::stable_sort(ord.begin(), ord.end(), [&](size_t a, size_t b) { return o_frame[a] != o_frame[b] ? o_frame[a] < o_frame[b] : o_cam[a] < o_cam[b]; });
  std::vector<int> pt(M), ccam(M), first(N + 1, 0);
  std::vector<double> z(2 * M + 2);
  {
    size_t q = 0;
    for (int f = 0; f < N; ++f) {
      first[f] = (int)q;
      while (q < M && o_frame[ord[q]] == f) { pt[q] = o_pt[ord[q]]; ccam[q] = o_cam[ord[q]]; z[2 * q] = o_z[2 * ord[q]]; z[2 * q + 1] = o_z[2 * ord[q] + 1]; ++q; }
    }
    first[N] = (int)M;
  }
  std::vector<double> corner((M + 1) * vc::kTrCornerStride, 0.0);
  std::vector<int> corner_ok(M + 1, 0);
  // the system over [d | s]
  std::vector<double> S((size_t)n * n, 0.0), Sds((size_t)n * vc::kSelMaxD, 0.0), gd(n, 0.0), Sss((size_t)vc::kSelMaxD * vc::kSelMaxD, 0.0), gs(vc::kSelMaxD, 0.0);
  std::vector<int> pcorners(P, 0);
  double cost = 0.0;
  for (int f = 0; f < N; ++f) {
    std::vector<double> G(vc::kSelGramDoubles), Hcc((size_t)vc::kSelMaxCams * 256, 0.0), Wf(6 * vc::kSelMaxD, 0.0), Y(6 * vc::kSelMaxD, 0.0), gsl(vc::kSelMaxD, 0.0);
    double Hff[36] = {0}, W16[96], tmp[24] = {0}, yr[6], fcost = 0.0;
    unsigned seen = 0;
    int corners = 0, behind = 0;
    for (int q = first[f]; q < first[f + 1];) {
      const int c = ccam[q];
      int q1 = q;
      while (q1 < first[f + 1] && ccam[q1] == c) ++q1;
      const double* cam = rig.cam + c * vc::kCamStride;
      vc::TileXf x;
      double K[10], Rck[9];
      vc::view_setup(T_wk + 7 * (size_t)f, cam, &x, K);
      vc::quat_to_R(cam, Rck);
      vc::ModelPre pre;
      vc::model_precompute(rig.model[c], K, &pre);
      int n_ok = 0, n_bad = 0;
      vc::with_model(rig.model[c], [&](auto m) {
        view_sweep<decltype(m)::value>(x, K, pre, Rck, rig.flags[c], points, &pt[q], &z[2 * (size_t)q], q1 - q, G.data(), &corner[(size_t)q * vc::kTrCornerStride], &corner_ok[q],
                                       &n_ok, &n_bad, &fcost);
      });
      corners += n_ok; behind += n_bad;
      if (n_ok > 0) {
        vc::sel_view_blocks(G.data(), cam, rig.model[c], rig.flags[c], Hff, W16, &Hcc[(size_t)c * 256], tmp);
        for (int j = 0; j < rig.ncols[c]; ++j) {
          for (int r = 0; r < 6; ++r) Wf[r * vc::kSelMaxD + rig.col0[c] + j] = W16[r * vc::kUCols + j];
          gsl[rig.col0[c] + j] = tmp[6 + j];
        }
        seen |= 1u << c;
      }
      q = q1;
    }
    double dinv[6];
    const bool chol_ok = corners >= 4 && vc::sel_chol6(Hff, dinv);
    const int status = vc::sel_frame_status(corners, behind, chol_ok);
    frame_status[3 * f] = status; frame_status[3 * f + 1] = corners; frame_status[3 * f + 2] = behind;
    if (!vc::sel_usable(status)) continue;
    cost += fcost;
    for (int j = 0; j < D; ++j) vc::sel_schur_col(Hff, dinv, Wf.data(), vc::kSelMaxD, j, &Y[j], vc::kSelMaxD);
    vc::sel_schur_col(Hff, dinv, tmp, 1, 0, yr, 1);
    for (int i = 0; i < D; ++i)
      for (int j = i; j < D; ++j) {
        const int ci = vc::sel_col_cam(rig, i), cj = vc::sel_col_cam(rig, j);
        const double hss = (ci == cj && ((seen >> ci) & 1u)) ? Hcc[(size_t)ci * 256 + (i - rig.col0[ci]) * vc::kUCols + (j - rig.col0[ci])] : 0.0;
        Sss[i * vc::kSelMaxD + j] += vc::sel_info_entry(hss, Y.data(), vc::kSelMaxD, i, j);
      }
    for (int j = 0; j < D; ++j) { double g = gsl[j]; for (int k = 0; k < 6; ++k) g -= Y[k * vc::kSelMaxD + j] * yr[k]; gs[j] -= g; }      // (g_s = -(J_s^T r - Y_s^T y_r))
    // the frame's (frame, point) records: the corners of a point by camera
    std::map<int, std::vector<int>> by_point;
    for (int q = first[f]; q < first[f + 1]; ++q) by_point[pt[q]].push_back(q);
    std::vector<int> rp;
    std::vector<double> recs;
    for (auto& kv : by_point) {
      double rec[vc::kTrRecStride] = {0};
      int nok = 0;
      for (int q : kv.second) { vc::tr_record_add(&corner[(size_t)q * vc::kTrCornerStride], rec); nok += corner_ok[q]; }
      vc::tr_record_solve(Hff, dinv, rec);
      pcorners[kv.first] += nok;
      rp.push_back(kv.first); recs.insert(recs.end(), rec, rec + vc::kTrRecStride);
      const int p = kv.first;
      for (int q : kv.second) {                                      // the columns of s: the corner's camera's own block
        const int c = ccam[q];
        for (int a = 0; a < 3; ++a)
          for (int j = 0; j < rig.ncols[c]; ++j) Sds[(size_t)(3 * p + a) * vc::kSelMaxD + rig.col0[c] + j] += corner[(size_t)q * vc::kTrCornerStride + vc::kTrCornerC + a * vc::kUCols + j];
      }
      for (int a = 0; a < 3; ++a) {
        for (int j = 0; j < D; ++j) Sds[(size_t)(3 * p + a) * vc::kSelMaxD + j] -= vc::tr_y_dot(rec + vc::kTrRecY, a, &Y[j], vc::kSelMaxD);
        gd[3 * p + a] -= rec[vc::kTrRecG + a] - vc::tr_y_dot(rec + vc::kTrRecY, a, yr, 1);
      }
    }
    for (size_t a = 0; a < rp.size(); ++a)
      for (size_t b = 0; b < rp.size(); ++b) {
        double acc[9] = {0};
        if (a == b) for (int e = 0; e < 9; ++e) acc[e] += recs[a * vc::kTrRecStride + vc::kTrRecP + e];
        vc::tr_pair_sub(&recs[a * vc::kTrRecStride + vc::kTrRecY], &recs[b * vc::kTrRecStride + vc::kTrRecY], acc);
        for (int i = 0; i < 3; ++i)
          for (int j = 0; j < 3; ++j) S[(size_t)(3 * rp[a] + i) * n + 3 * rp[b] + j] += acc[i * 3 + j];
      }
  }
  for (int p = 0; p < P; ++p) { point_corners[p] = pcorners[p]; point_status[p] = pcorners[p] > 0 ? vc::kTrPointOk : vc::kTrPointUnobserved; }
  *result_status = vc::kTrSingular; *gauge_rank = 0;
  // the shared columns eliminated
  if (D > 0) {
    std::vector<double> U((size_t)D * D, 0.0), cs(D), zg(D);
    for (int j = 0; j < D; ++j) cs[j] = vc::sel_scale(Sss[j * vc::kSelMaxD + j]);
    for (int i = 0; i < D; ++i)
      for (int j = i; j < D; ++j) U[i * D + j] = vc::sel_scaled(Sss[i * vc::kSelMaxD + j], cs[i], cs[j]) + (i == j ? vc::kTrPriorS : 0.0);
    for (int k = 0; k + 1 < D; ++k)
      for (int j = k + 1; j < D; ++j) vc::sel_chol_step(U.data(), D, k, j);
    for (int k = 0; k < D; ++k) if (!(U[k * D + k] > 0.0)) return 0;
    for (int k = 0; k < D; ++k) zg[k] = vc::tr_fwd_entry(U.data(), D, k, cs[k] * gs[k], zg.data());
    for (int k = 0; k < D; ++k) zg[k] *= std::sqrt(U[k * D + k]);
    for (int i = 0; i < n; ++i) {
      double* row = &Sds[(size_t)i * vc::kSelMaxD];
      for (int k = 0; k < D; ++k) row[k] = vc::tr_fwd_entry(U.data(), D, k, cs[k] * row[k], row);
      for (int k = 0; k < D; ++k) row[k] *= std::sqrt(U[k * D + k]);
    }
    for (int i = 0; i < n; ++i) {
      for (int j = 0; j < n; ++j) { double s = 0.0; for (int k = 0; k < D; ++k) s += Sds[(size_t)i * vc::kSelMaxD + k] * Sds[(size_t)j * vc::kSelMaxD + k]; S[(size_t)i * n + j] -= s; }
      double t = 0.0;
      for (int k = 0; k < D; ++k) t += Sds[(size_t)i * vc::kSelMaxD + k] * zg[k];
      gd[i] -= t;
    }
  }
  // gauge and prior over the observed points
  std::vector<int> live(n, 0);
  int n_obs = 0;
  double cen[3] = {0, 0, 0};
  for (int p = 0; p < P; ++p)
    if (point_status[p] == vc::kTrPointOk) { ++n_obs; for (int a = 0; a < 3; ++a) { live[3 * p + a] = 1; cen[a] += nominal[3 * p + a]; } }
  if (n_obs == 0) return 0;
  for (int a = 0; a < 3; ++a) cen[a] /= n_obs;
  std::vector<std::vector<double>> Q;
  for (int c = 0; c < vc::kTrGaugeCols; ++c) {
    std::vector<double> q(n, 0.0);
    for (int i = 0; i < n; ++i)
      if (live[i]) { const int p = i / 3; const double u[3] = {nominal[3 * p] - cen[0], nominal[3 * p + 1] - cen[1], nominal[3 * p + 2] - cen[2]}; q[i] = vc::tr_gauge_entry(c, i - 3 * p, u); }
    auto dot = [&](const std::vector<double>& a, const std::vector<double>& b) { double s = 0.0; for (int i = 0; i < n; ++i) s += a[i] * b[i]; return s; };
    const double before = std::sqrt(dot(q, q));
    for (auto& k : Q) { const double d = dot(k, q); for (int i = 0; i < n; ++i) q[i] -= d * k[i]; }
    const double after = std::sqrt(dot(q, q));
    if (vc::tr_gauge_keep(after, before)) { for (double& x : q) x /= after; Q.push_back(q); }
  }
  *gauge_rank = (int)Q.size();
  auto project = [&](std::vector<double>& x) {
    std::vector<double> t(Q.size());
    for (size_t c = 0; c < Q.size(); ++c) { double s = 0.0; for (int i = 0; i < n; ++i) s += Q[c][i] * x[i]; t[c] = s; }
    for (int i = 0; i < n; ++i) { double s = x[i]; for (size_t c = 0; c < Q.size(); ++c) s -= Q[c][i] * t[c]; x[i] = live[i] ? s : 0.0; }
  };
  std::vector<double> pe(n, 0.0), rhs(n, 0.0);
  for (int i = 0; i < n; ++i) if (live[i]) pe[i] = points[i] - nominal[i];
  project(pe);
  double trace = 0.0;
  for (int i = 0; i < n; ++i) if (live[i]) { rhs[i] = gd[i] - lambda * pe[i]; trace += S[(size_t)i * n + i] + lambda; }
  project(rhs);
  const double mu = trace / (3.0 * n_obs);
  const int nq = (int)Q.size();
  std::vector<double> V((size_t)nq * n, 0.0), G7((size_t)nq * nq, 0.0);
  for (int c = 0; c < nq; ++c)
    for (int i = 0; i < n; ++i) {
      if (!live[i]) continue;
      double s = 0.0;
      for (int j = 0; j < n; ++j) if (live[j]) s += (S[(size_t)j * n + i] + (i == j ? lambda : 0.0)) * Q[c][j];
      V[(size_t)c * n + i] = s;
    }
  for (int a = 0; a < nq; ++a)
    for (int b = 0; b < nq; ++b) { double s = 0.0; for (int i = 0; i < n; ++i) s += Q[a][i] * V[(size_t)b * n + i]; G7[a * nq + b] = s; }
  for (int i = 0; i < n; ++i) {
    std::vector<double> r(nq);
    for (int c = 0; c < nq; ++c) {
      double s = 0.0;
      for (int a = 0; a < nq; ++a) s += Q[a][i] * (0.5 * (G7[a * nq + c] + G7[c * nq + a]) + (a == c ? mu : 0.0));
      r[c] = V[(size_t)c * n + i] - 0.5 * s;
    }
    for (int c = 0; c < nq; ++c) V[(size_t)c * n + i] = r[c];
  }
  std::vector<double> A((size_t)n * n, 0.0);
  double top = 0.0;
  for (int i = 0; i < n; ++i)
    for (int j = 0; j < n; ++j) {
      double a = i == j ? 1.0 : 0.0;
      if (live[i] && live[j]) {
        double s = 0.0;
        for (int c = 0; c < nq; ++c) s += Q[c][i] * V[(size_t)c * n + j] + V[(size_t)c * n + i] * Q[c][j];
        a = S[(size_t)i * n + j] + (i == j ? lambda : 0.0) - s;
        if (i == j && a > top) top = a;
      }
      A[(size_t)i * n + j] = a;
    }
  // dense Cholesky (lower, in place) with the pivot rule, and the two triangular solves
  for (int j = 0; j < n; ++j) {
    double d = A[(size_t)j * n + j];
    for (int k = 0; k < j; ++k) d -= A[(size_t)j * n + k] * A[(size_t)j * n + k];
    if (live[j] && !vc::tr_pivot_ok(d, top)) return 0;
    const double l = std::sqrt(d);
    A[(size_t)j * n + j] = l;
    for (int i = j + 1; i < n; ++i) {
      double s = A[(size_t)i * n + j];
      for (int k = 0; k < j; ++k) s -= A[(size_t)i * n + k] * A[(size_t)j * n + k];
      A[(size_t)i * n + j] = s / l;
    }
  }
  std::vector<double> x(rhs);
  for (int i = 0; i < n; ++i) { double s = x[i]; for (int k = 0; k < i; ++k) s -= A[(size_t)i * n + k] * x[k]; x[i] = s / A[(size_t)i * n + i]; }
  for (int i = n - 1; i >= 0; --i) { double s = x[i]; for (int k = i + 1; k < n; ++k) s -= A[(size_t)k * n + i] * x[k]; x[i] = s / A[(size_t)i * n + i]; }
  double pred = 0.0;
  for (int i = 0; i < n; ++i) { pred += x[i] * rhs[i]; refined[i] = live[i] ? nominal[i] + pe[i] + x[i] : points[i]; }
  *cost_out = 0.5 * cost; *pred_out = 0.5 * pred; *result_status = vc::kTrOk;
  return 0;
}

}  // extern "C"

#ifdef TARGET_REFINE_HARNESS_MAIN
// a 3 x 3 board seen by a linear camera from four poses, one corner dropped: runs the whole step once and prints the result
int main() {
  const int model[1] = {vc::kLinear}, flags[1] = {vc::kCamKFree};
  const double params[10] = {420.0, 420.0, 320.0, 240.0}, T_ck[7] = {0, 0, 0, 1, 0, 0, 0};
  const int N = 4, P = 9;
  double T_wk[7 * N], points[3 * P], nominal[3 * P];
  for (int p = 0; p < P; ++p) {
    nominal[3 * p] = 0.03 * (p % 3 - 1); nominal[3 * p + 1] = 0.03 * (p / 3 - 1); nominal[3 * p + 2] = 0.0;
    for (int a = 0; a < 3; ++a) points[3 * p + a] = nominal[3 * p + a];
  }
  std::vector<int> tile_frame, tile_cam, point_id;
  std::vector<long long> tile_off(1, 0);
  std::vector<double> p_c;
  for (int f = 0; f < N; ++f) {
    const double ang = 0.2 * (f + 1), half = 0.5 * ang, axis[3] = {f % 2 ? 1.0 : 0.0, f % 2 ? 0.0 : 1.0, 0.0};
    double* T = T_wk + 7 * f;
    T[0] = axis[0] * std::sin(half); T[1] = axis[1] * std::sin(half); T[2] = 0.0; T[3] = std::cos(half);
    double R[9];
    vc::quat_to_R(T, R);
    for (int a = 0; a < 3; ++a) T[4 + a] = -R[3 * a + 2] * 0.4;
    vc::TileXf x;
    double K[10];
    double cam[vc::kCamStride] = {0};
    std::memcpy(cam, T_ck, 56); std::memcpy(cam + vc::kCamK, params, 32);
    vc::view_setup(T, cam, &x, K);
    vc::ModelPre pre;
    vc::model_precompute(vc::kLinear, K, &pre);
    tile_frame.push_back(f); tile_cam.push_back(0);
    for (int p = 0; p < P; ++p) {
      if (f == 1 && p == 4) continue;
      const double bowed[3] = {nominal[3 * p] * 1.002, nominal[3 * p + 1], 0.5 * nominal[3 * p] * nominal[3 * p]};
      double pc[3], pix[2];
      vc::tile_point(x, bowed, pc);
      vc::project_any<false>(vc::kLinear, pc, K, pre, pix, nullptr, nullptr);
      point_id.push_back(p); p_c.push_back(pix[0]); p_c.push_back(pix[1]);
    }
    tile_off.push_back((long long)point_id.size());
  }
  double refined[3 * P], cost = 0, pred = 0;
  int pstat[P], pcorners[P], fstat[3 * N], rank = 0, status = -1;
  const int rc = vch_target_refine(1, model, params, T_ck, flags, N, T_wk, N, tile_frame.data(), tile_cam.data(), tile_off.data(), point_id.data(), p_c.data(), points, nominal, P,
                                   1e4, refined, pstat, pcorners, fstat, &rank, &status, &cost, &pred);
  std::printf("rc %d status %d rank %d cost %.6e predicted decrease %.6e\n", rc, status, rank, cost, pred);
  for (int p = 0; p < P; ++p) std::printf("  %d: %+.6e %+.6e %+.6e (%d corners)\n", p, refined[3 * p] - nominal[3 * p], refined[3 * p + 1] - nominal[3 * p + 1], refined[3 * p + 2], pcorners[p]);
  return rc == 0 && status == 0 && rank == 7 && pred >= 0.0 ? 0 : 1;
}
#endif
