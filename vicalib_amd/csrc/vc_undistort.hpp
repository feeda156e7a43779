// vc_undistort.hpp -- the arithmetic the undistortion kernels (vc_undistort.hip) share with the host code that fits the destination
// intrinsics (vc_undistort_fit_linear): a destination pixel's ray into the source image, and the inverse -- a distorted source
// pixel back to its ray.  All projection goes through model_precompute / project_any (vc_math.hpp); nothing here restates a camera
// formula.  The inverse runs Newton on the model's radial profile r_d = f(r_u) (theta for kb4), with both f and f' read from ONE
// call of project_any<true> on a point of the x axis at unit focal length: the pixel is f, the Jacobian A is the slope.
#pragma once
#include "vc_math.hpp"

namespace vc {

// a coordinate this close outside [0, w - 1] x [0, h - 1] is ON the border (clamped onto it), not outside: the map's own arithmetic
// ((i - u0) / fu) * fu + u0 leaves the last destination column of an identity map at w - 1 + 1e-13 as often as at w - 1
constexpr double kUndistBorderTol = 1e-9;
constexpr int kUndistNewtonIters = 40;
constexpr double kUndistNewtonTol = 1e-14;

struct UndistPlan {
  int model, src_w, src_h, dst_w, dst_h;
  int map_pitch;            // entries per map row: dst_w rounded up to 4 (rows of the map start 32-byte aligned)
  int fill;
  int pad_;
  double K[10];             // source model [fu fv u0 v0 distortion...]
  ModelPre pre;
  double dl[4];             // destination pinhole fu fv u0 v0
  double R_sd[9];           // destination-camera ray -> source-camera ray (row-major); R_ds = R_sd^T
};

// source pixel of destination pixel (i, j); false = no source pixel (see k_undist_map for the three cases)
VC_HD bool undist_map_entry(const UndistPlan& p, int i, int j, double* x, double* y) {
  const double a = ((double)i - p.dl[2]) / p.dl[0], b = ((double)j - p.dl[3]) / p.dl[1];
  const double* R = p.R_sd;
  const double ray[3] = {R[0] * a + R[1] * b + R[2], R[3] * a + R[4] * b + R[5], R[6] * a + R[7] * b + R[8]};
  if (!(ray[2] > 0.0) && p.model != kKb4) return false;
  double pix[2];
  project_any<false>(p.model, ray, p.K, p.pre, pix, nullptr, nullptr);
  const double xm = (double)(p.src_w - 1), ym = (double)(p.src_h - 1);
  // (one comparison chain: a NaN or an infinity fails it)
  if (!(pix[0] >= -kUndistBorderTol && pix[0] <= xm + kUndistBorderTol && pix[1] >= -kUndistBorderTol && pix[1] <= ym + kUndistBorderTol)) return false;
  *x = fmin(fmax(pix[0], 0.0), xm);
  *y = fmin(fmax(pix[1], 0.0), ym);
  return true;
}

// the radial profile at unit focal length and its slope: t = r_u = tan(angle off the axis), or the angle itself for kb4
VC_HD void undist_profile(int model, const double* Kn, const ModelPre& pre, double t, double* f, double* df) {
  double pc[3] = {t, 0.0, 1.0}, pix[2], A[6], B[20];
  if (model == kKb4) { pc[0] = sin(t); pc[2] = cos(t); }
  project_any<true>(model, pc, Kn, pre, pix, A, B);
  *f = pix[0];
  *df = model == kKb4 ? A[0] * pc[2] - A[2] * pc[0] : A[0];      // d/dt along (sin t, 0, cos t) for kb4, d/dX at Z = 1 otherwise
}

// distorted source pixel (u, v) -> its ray in the source camera's frame; false: the pixel is beyond the model's image (the iteration
// does not converge in kUndistNewtonIters steps, leaves the positive range or meets a non-positive slope)
VC_HD bool undist_unproject(int model, const double* K, const ModelPre& pre, double u, double v, double* ray) {
  double Kn[10];
  Kn[0] = 1.0; Kn[1] = 1.0; Kn[2] = 0.0; Kn[3] = 0.0;
  for (int k = 4; k < 10; ++k) Kn[k] = K[k];
  const double xd = (u - K[2]) / K[0], yd = (v - K[3]) / K[1];
  const double rd = sqrt(xd * xd + yd * yd);
  if (!(rd >= 0.0) || !(rd <= 1e300)) return false;
  double t = rd;
  bool ok = false;
  for (int it = 0; it < kUndistNewtonIters; ++it) {
    double f, df;
    undist_profile(model, Kn, pre, t, &f, &df);
    if (!(df > 0.0)) return false;
    const double res = f - rd;
    if (fabs(res) <= kUndistNewtonTol * (1.0 + rd)) { ok = true; break; }
    t -= res / df;
    if (!(t >= 0.0) || (model == kKb4 && t > 3.14159265358979323846)) return false;
  }
  if (!ok) return false;
  const double ird = rd > 0.0 ? 1.0 / rd : 0.0;
  if (model == kKb4) {
    const double s = sin(t);
    ray[0] = s * xd * ird; ray[1] = s * yd * ird; ray[2] = cos(t);
  } else {
    ray[0] = t * xd * ird; ray[1] = t * yd * ird; ray[2] = 1.0;
  }
  return true;
}

// ... and on through R_ds = R_sd^T into the destination pinhole camera; false also for a ray with z <= 0 there or a result that is not finite
VC_HD bool undist_point(const UndistPlan& p, double u, double v, double* ou, double* ov) {
  double r[3];
  if (!undist_unproject(p.model, p.K, p.pre, u, v, r)) return false;
  const double* R = p.R_sd;
  const double x = R[0] * r[0] + R[3] * r[1] + R[6] * r[2], y = R[1] * r[0] + R[4] * r[1] + R[7] * r[2], z = R[2] * r[0] + R[5] * r[1] + R[8] * r[2];
  if (!(z > 0.0)) return false;
  const double a = p.dl[0] * (x / z) + p.dl[2], b = p.dl[1] * (y / z) + p.dl[3];
  if (!(fabs(a) <= 1e300 && fabs(b) <= 1e300)) return false;
  *ou = a; *ov = b;
  return true;
}

// orthonormal to 1e-9 with a positive determinant: what a caller's rotation matrix (row-major) is held to
inline bool is_rotation(const double* R) {
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) {
      const double d = R[3 * i] * R[3 * j] + R[3 * i + 1] * R[3 * j + 1] + R[3 * i + 2] * R[3 * j + 2] - (i == j ? 1.0 : 0.0);
      if (!(std::fabs(d) <= 1e-9)) return false;
    }
  const double det = R[0] * (R[4] * R[8] - R[5] * R[7]) - R[1] * (R[3] * R[8] - R[5] * R[6]) + R[2] * (R[3] * R[7] - R[4] * R[6]);
  return det > 0.0;
}

}  // namespace vc

// ---- host side of vc_undistort.hip that the rectifier (vc_rectify.hip) builds on; defined there
struct vc_undistorter;
namespace vc {
// model, K, pre, source size and R_sd = R_ds^T (NULL = identity) of a plan; everything else zero
void undist_source_plan(UndistPlan* p, int model, const double* params, int nparams, int src_w, int src_h, const double* R_ds);
// one destination camera for n_sides sources (vc_undistort_fit_linear: one side; vc_stereo_fit_linear: two); a status of the C ABI
int undist_fit_sides(int n_sides, UndistPlan* side, int dst_w, int dst_h, double alpha, double dst_linear[4]);
bool undist_source_args_ok(int model, const double* params, int nparams, int w, int h);      // the checks of vc_undistorter_create
bool undist_dest_args_ok(const double* dst_linear /* nullable */, int dst_w, int dst_h, int fill);
const UndistPlan& undist_plan_of(const vc_undistorter* u);
// vc_undistort_images in two halves: everything enqueued on the handle's stream / the wait and the copy to the caller
int undist_images_begin(vc_undistorter* u, int n, const unsigned char* src, int src_pitch, long long src_stride, unsigned char* dst, int dst_pitch, long long dst_stride);
int undist_images_end(vc_undistorter* u, int n, unsigned char* dst, int dst_pitch, long long dst_stride);
}  // namespace vc
