// TEST INFRASTRUCTURE: the arithmetic of the stereo uncertainty map (vicalib_amd/csrc/vc_stereo_uncertainty.hpp, VC_HD, and rect_pose_jacobian of
// vc_rectify.hpp) compiled for the host, so that the CPU suite can hold the pose Jacobian, the sides' blocks and the map against numpy without a
// GPU.  The argument check, the map onto eta and the packing of the covariance are the very functions the library runs; what the kernels add is
// the indexing and the order of the sums, which are plain loops in sample order here.
#include <cmath>
#include <cstring>
#include <vector>
#include "../../vicalib_amd/csrc/vc_stereo_uncertainty.hpp"

extern "C" {

// the shared argument check of a run on its own
int vch_su_args_ok(const double* cov, int n, double sigma_px, const double* depths, int n_depths) { return vc::su_run_args_ok(cov, n, sigma_px, depths, n_depths) ? 1 : 0; }

// W (7 x 12) of rect_pose_jacobian: 0, 1 (coincident), 2 (vertical) or -2 (a pose that is not one)
int vch_su_pose_jacobian(const double* T_ck_a, const double* T_ck_b, double* W) {
  double Ta[7], Tb[7];
  if (!vc::pose_ok(T_ck_a, Ta) || !vc::pose_ok(T_ck_b, Tb)) return -2;
  return vc::rect_pose_jacobian(Ta, Tb, W);
}

// One whole run.  var = n_depths x n x 3; flags = n_depths x n; summary = n_depths x [count, invalid, sum var_dv, sum var_d, sum var_Z,
// max var_dv, worst]; pose_var = 7.  Returns 0, -2 (VC_ERR_BAD_ARG), -6 (coincident) or -7 (vertical).
int vch_stereo_uncertainty(int model_a, const double* Ka, int nka, int w_a, int h_a, const double* T_ck_a, int model_b, const double* Kb, int nkb, int w_b, int h_b,
                           const double* T_ck_b, const double* dst_linear, int dst_w, int dst_h, int gx, int gy, const double* cov, double sigma_px,
                           const double* depths, int n_depths, double* var, unsigned char* flags, double* summary, double* pose_var) {
  double Ta[7], Tb[7], W[84];
  if (!vc::cvt_model_ok(model_a) || nka != vc::model_nk(model_a) || !vc::cvt_model_ok(model_b) || nkb != vc::model_nk(model_b)) return -2;
  if (!dst_linear || !vc::cvt_grid_ok(dst_w, dst_h, gx, gy) || !vc::pose_ok(T_ck_a, Ta) || !vc::pose_ok(T_ck_b, Tb)) return -2;
  const int n_cov = 14 + nka + nkb;
  if (!vc::su_run_args_ok(cov, n_cov, sigma_px, depths, n_depths)) return -2;
  vc::SuPlan p;
  std::memset(&p, 0, sizeof(p));
  const int rc = vc::rectify_rotations(Ta, Tb, p.R_ds[0], p.R_ds[1], &p.baseline);
  if (rc != vc::kRectOk) return rc == vc::kRectCoincident ? -6 : -7;
  vc::rect_pose_jacobian(Ta, Tb, W);
  vc::cmp_plan_set(&p.lat, model_a, Ka, nka, model_b, Kb, nkb, dst_w, dst_h, gx, gy);
  std::memcpy(p.dl, dst_linear, 32);
  p.src_w[0] = w_a; p.src_h[0] = h_a; p.src_w[1] = w_b; p.src_h[1] = h_b;
  double T[vc::kSuEta * vc::kSuMaxCov];
  vc::SuCov pc;
  vc::su_eta_map(Ta, Tb, nka, nkb, W, T);
  vc::su_pack_cov(cov, n_cov, T, sigma_px, &pc);
  for (int k = 0; k < 7; ++k) pose_var[k] = pc.P[vc::su_pidx(k, k)];
  const int n = p.lat.n;
  for (int d = 0; d < n_depths; ++d) {
    double* sum = summary + 7 * d;
    for (int k = 0; k < 7; ++k) sum[k] = 0.0;
    double best = -1.0; long long best_i = -1;
    for (int s = 0; s < n; ++s) {
      double r[3], blk[2][vc::kSuSideDoubles], v[3];
      bool ok[2];
      for (int side = 0; side < 2; ++side) {
        vc::su_point(p, s, depths[d], side, r);
        vc::with_model(side ? model_b : model_a, [&](auto m) {
          ok[side] = vc::su_side_block<decltype(m)::value>(side ? p.lat.Kb : p.lat.Ka, side ? p.lat.pre_b : p.lat.pre_a, p.src_w[side], p.src_h[side], p.R_ds[side], p.dl, r,
                                                           blk[side]);
        });
      }
      const bool valid = ok[0] && ok[1] && vc::su_variances(blk[0], blk[1], p.dl[0], depths[d], p.baseline, pc.P, v);
      double* dst = var + ((size_t)d * n + s) * 3;
      for (int k = 0; k < 3; ++k) dst[k] = valid ? v[k] : NAN;
      flags[(size_t)d * n + s] = (unsigned char)((ok[0] ? 0 : vc::kCmpFlagA) | (ok[1] ? 0 : vc::kCmpFlagB) | (valid ? 0 : vc::kCmpFlagInvalid));
      if (!valid) { sum[1] += 1.0; continue; }
      sum[0] += 1.0; sum[2] += v[0]; sum[3] += v[1]; sum[4] += v[2];
      if (v[0] > best) { best = v[0]; best_i = s; }
    }
    sum[5] = best_i >= 0 ? best : 0.0; sum[6] = (double)best_i;
  }
  return 0;
}

}  // extern "C"
