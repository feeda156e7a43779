// vc_dot_bias.hpp -- the arithmetic of the predicted centre bias of a dot (vc_dot_bias.hip: vc_dot_bias_batch), shared with the host build of
// tests/host_harness/dot_bias_harness.cpp.  A measurement is the centre of a dot's image ellipse as the detector's dual-conic fit returns it
// (vc_detect.hip: k_det_fit); the solve holds it against project(centre of the circle).  Under perspective and lens distortion the two differ.
// The predicted bias is what the detector's own estimator returns in the noise-free, blur-free limit minus the projection of the circle's centre.
// The lane group W is that of vc_seed.hpp: the wavefront on the device, SeedSerial on the host.
//   circle        centre C on the target, radius r, in the plane through C parallel to the target's x-y plane; T_cw = [q | t], R = R(q)
//   centre        p0, A0 = project_any<true>(R C + t)
//   scale         s = r sqrt((|A0 R e_x|^2 + |A0 R e_y|^2) / 2): the dot's radius in pixels to first order (the same in every lane, no sum)
//   samples       64, sample i in lane i on the device: a_i = 2 pi (i + 0.5) / 64, P_i = C + r (cos a_i e_x + sin a_i e_y),
//                 tangent T_i = -sin a_i e_x + cos a_i e_y; pix_i, A_i = project_any<true>(R P_i + t)
//   edge line     q_i = (pix_i - p0) / s, d_i = A_i R T_i, n_i = (-d_y, d_x) / |d_i|, l_i = (a, b, c) = (n_x, n_y, -n_i . q_i)
//   fit           the detector's equations with unit weights (vc_conic5.hpp): sum K_i K_i^T theta = -sum K_i c_i^2; the twenty sums in the
//                 lane group's fixed order; bias = s (theta_3, theta_4) / 2
//   status        1 the centre does not project (the PnP code's rule for a corner: depth <= 1e-9, a pixel that is not finite; also a scale
//                 that is not finite); 2 a boundary sample does not project, or |d_i| is zero or not finite; 3 the 5 x 5 system is singular
//                 or the bias is not finite; 4 |bias| > s: the estimate left the dot, the view is too oblique to trust
//   r == 0        behind the centre's test: bias exactly (0, 0), radius_px 0, status 0
#pragma once
#include "vc_seed.hpp"
#include "vc_conic5.hpp"

namespace vc {

enum DotBiasStatus { kDotBiasOk = 0, kDotBiasNoCentre = 1, kDotBiasNoRim = 2, kDotBiasSingular = 3, kDotBiasLeftDot = 4 };
constexpr int kDotBiasSamples = 64;

// the camera of a view and its pose, ready for the observations of that view
struct DotBiasView {
  int model;
  double K[10];
  ModelPre pre;
  double R[9], t[3];
};
VC_HD void dot_bias_view(int model, const double* K /*10*/, const double* T_cw /*7*/, DotBiasView* v) {
  v->model = model;
  VC_SEED_UNROLL
  for (int k = 0; k < 10; ++k) v->K[k] = K[k];
  model_precompute(model, v->K, &v->pre);
  quat_to_R(T_cw, v->R);
  v->t[0] = T_cw[4]; v->t[1] = T_cw[5]; v->t[2] = T_cw[6];
}

// pixel and d pix / d p_c (2 x 3) of the target point P; false where seed_cost refuses a corner
VC_HD bool dot_bias_project(const DotBiasView& v, const double* P, double* pix, double* A) {
  double pc[3], B[20];
  VC_SEED_UNROLL
  for (int a = 0; a < 3; ++a) pc[a] = v.R[3 * a] * P[0] + v.R[3 * a + 1] * P[1] + v.R[3 * a + 2] * P[2] + v.t[a];
  if (!(pc[2] > 1e-9)) return false;                     // (a NaN depth fails the comparison)
  project_any<true>(v.model, pc, v.K, v.pre, pix, A, B);
  return seed_finite(pix[0]) && seed_finite(pix[1]);
}
// A R e: the image of the target direction e = ex e_x + ey e_y
VC_HD void dot_bias_direction(const DotBiasView& v, const double* A, double ex, double ey, double* d) {
  double g[3];
  VC_SEED_UNROLL
  for (int a = 0; a < 3; ++a) g[a] = v.R[3 * a] * ex + v.R[3 * a + 1] * ey;
  d[0] = A[0] * g[0] + A[1] * g[1] + A[2] * g[2];
  d[1] = A[3] * g[0] + A[4] * g[1] + A[5] * g[2];
}

// One observation.  The status, the same in every lane; with kDotBiasOk bias (2) and *radius_px are set, the same in every lane.
template <class W>
VC_HD int dot_bias_one(const W& w, const DotBiasView& v, const double* C, double r, double* bias, double* radius_px) {
  double p0[2], A0[6], dx[2], dy[2];
  if (!dot_bias_project(v, C, p0, A0)) return kDotBiasNoCentre;
  dot_bias_direction(v, A0, 1.0, 0.0, dx);
  dot_bias_direction(v, A0, 0.0, 1.0, dy);
  const double s = r * sqrt(0.5 * (dx[0] * dx[0] + dx[1] * dx[1] + dy[0] * dy[0] + dy[1] * dy[1]));
  if (!seed_finite(s)) return kDotBiasNoCentre;
  if (r == 0.0) { bias[0] = 0.0; bias[1] = 0.0; *radius_px = 0.0; return kDotBiasOk; }
  double acc[20];
  VC_SEED_UNROLL
  for (int k = 0; k < 20; ++k) acc[k] = 0.0;
  int bad = 0;
  for (int i = w.lane; i < kDotBiasSamples; i += W::kLanes) {
    const double ang = (2.0 * 3.14159265358979323846 / kDotBiasSamples) * (i + 0.5);
    const double ca = cos(ang), sa = sin(ang);
    const double P[3] = {C[0] + r * ca, C[1] + r * sa, C[2]};
    double pix[2], A[6], d[2];
    if (!dot_bias_project(v, P, pix, A)) { ++bad; continue; }
    dot_bias_direction(v, A, -sa, ca, d);
    const double dn = sqrt(d[0] * d[0] + d[1] * d[1]);
    if (!(dn > 0.0) || !seed_finite(dn)) { ++bad; continue; }
    const double a = -d[1] / dn, b = d[0] / dn;
    const double c = -(a * ((pix[0] - p0[0]) / s) + b * ((pix[1] - p0[1]) / s));
    const double Kk[5] = {a * a, a * b, b * b, a * c, b * c};
    int e = 0;
    VC_SEED_UNROLL
    for (int m = 0; m < 5; ++m) {
      VC_SEED_UNROLL
      for (int n = m; n < 5; ++n) acc[e++] += Kk[m] * Kk[n];
    }
    VC_SEED_UNROLL
    for (int m = 0; m < 5; ++m) acc[15 + m] += Kk[m] * (-(c * c));
  }
  if (w.allsum(bad) > 0) return kDotBiasNoRim;
  VC_SEED_UNROLL
  for (int k = 0; k < 20; ++k) acc[k] = w.allsum(acc[k]);      // (all lanes, fixed order)
  double th[5];
  if (!conic5_solve(acc, th)) return kDotBiasSingular;
  const double bu = 0.5 * s * th[3], bv = 0.5 * s * th[4];
  if (!seed_finite(bu) || !seed_finite(bv)) return kDotBiasSingular;
  if (bu * bu + bv * bv > s * s) return kDotBiasLeftDot;
  bias[0] = bu; bias[1] = bv; *radius_px = s;
  return kDotBiasOk;
}

// ---- the host side of vc_dot_bias.hip ---------------------------------------------------------------------------------------------
// The arguments are those of vc_dot_bias_batch, already checked.  kernel_ms (nullable): the mean time of the kernel alone over time_reps
// more launches on the same input, back to back between two events.
int dot_bias_run(int device, int n_views, const int* view_model, const double* view_K, const double* view_T_cw, const int* view_off, const double* p_w,
                 const double* radius, double* bias, double* radius_px, int* status, int time_reps = 0, double* kernel_ms = nullptr);
bool dot_bias_args_ok(int n_views, const int* view_model, const double* view_K, const double* view_T_cw, const int* view_off, const double* p_w,
                      const double* radius, const double* bias, const double* radius_px, const int* status);

}  // namespace vc
