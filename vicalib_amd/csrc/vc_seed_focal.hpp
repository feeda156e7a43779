// vc_seed_focal.hpp -- the arithmetic of the focal-length seed (vc_seed_focal.hip: vc_seed_focal_batch), shared with the host build of
// tests/host_harness/seed_focal_harness.cpp.  Every view of the planar target gives a homography H from target (X, Y) to pixels relative to the
// assumed principal point; with square pixels and that principal point H = lambda K [r1 r2 t], K = diag(f, f, 1), and the orthonormality of r1
// and r2 gives two equations that are linear in a = 1 / f^2 (Zhang's constraints).  The lane group W is that of vc_seed.hpp: the wavefront on
// the device, SeedSerial on the host.
//   used corner   both coordinates finite and (u - cx)^2 + (v - cy)^2 <= R^2 (R <= 0: every finite corner)
//   status        1 fewer than max(min_corners, 4) used corners; 2 the used target points are not on one plane z = z0 (seed_view's rule, z0
//                 the first used corner's); 3 the DLT failed or H is not finite; 4 the rms transfer error of H exceeds max_fit_px (> 0)
//   rows          H scaled to h1x^2 + h1y^2 + h2x^2 + h2y^2 = 2 (h1, h2 its first two columns):
//                 c1 = h1x h2x + h1y h2y, d1 = -h1z h2z;  c2 = (h1x^2 + h1y^2) - (h2x^2 + h2y^2), d2 = h2z^2 - h1z^2;  c1 a = d1, c2 a = d2
//                 for an exact pinhole c1^2 + c2^2 is about sin^4(tilt): a fronto-parallel view weighs nothing
//   camera        over its status-0 views in view order Scc = sum(c1^2 + c2^2), Scd = sum(c1 d1 + c2 d2); f = sqrt(Scc / Scd)
//                 status 1 no usable view, 2 Scc < sin^4(min_tilt), 3 Scd / Scc not positive or not finite
#pragma once
#include "vc_seed.hpp"

namespace vc {

enum FocalViewStatus { kFocalOk = 0, kFocalFewCorners = 1, kFocalNotPlanar = 2, kFocalNoH = 3, kFocalBadFit = 4 };
enum FocalCamStatus { kFocalCamOk = 0, kFocalCamNoView = 1, kFocalCamNoTilt = 2, kFocalCamNoFocal = 3 };

struct FocalView {
  int n;
  const double* pw;      // n x 3
  const double* uv;      // n x 2
  double cx, cy, R;
};
struct FocalViewOut {
  double H[9], rows[4], f, fit_px;
  int used;
};

// the used corners of a view for seed_dlt_H: target (X, Y) against the pixel relative to the principal point
struct FocalPoints {
  const FocalView& s;
  VC_HD bool operator()(int i, double* X, double* Y, double* x, double* y) const {
    const double u = s.uv[2 * (size_t)i], v = s.uv[2 * (size_t)i + 1];
    *X = s.pw[3 * (size_t)i]; *Y = s.pw[3 * (size_t)i + 1];
    *x = u - s.cx; *y = v - s.cy;
    if (!seed_finite(u) || !seed_finite(v)) return false;
    return !(s.R > 0.0) || *x * *x + *y * *y <= s.R * s.R;
  }
};

VC_HD double focal_sin4(double min_tilt_deg) {
  const double sn = sin(min_tilt_deg * (3.14159265358979323846 / 180.0));
  return sn * sn * sn * sn;
}

// One view.  The status, the same in every lane; with kFocalOk *o is set, the same in every lane.
template <class W>
VC_HD int focal_view(const W& w, const FocalView& s, int min_corners, double max_fit_px, double sin4, FocalViewOut* o) {
  const FocalPoints pt{s};
  int m = 0, first = 0x7fffffff;
  for (int i = w.lane; i < s.n; i += W::kLanes) {
    double X, Y, x, y;
    if (pt(i, &X, &Y, &x, &y)) { ++m; if (i < first) first = i; }
  }
  m = w.allsum(m);
  if (m < (min_corners > 4 ? min_corners : 4)) return kFocalFewCorners;
  first = w.allmin(first);
  const double z0 = s.pw[3 * (size_t)first + 2];
  int off_plane = 0;
  for (int i = w.lane; i < s.n; i += W::kLanes) {
    double X, Y, x, y;
    if (pt(i, &X, &Y, &x, &y) && !(fabs(s.pw[3 * (size_t)i + 2] - z0) <= 1e-9)) ++off_plane;
  }
  if (w.allsum(off_plane) > 0) return kFocalNotPlanar;
  double H[9];
  if (!seed_dlt_H(w, s.n, pt, H)) return kFocalNoH;
  double hsum = 0.0;
  for (int k = 0; k < 9; ++k) hsum += fabs(H[k]);
  if (!seed_finite(hsum)) return kFocalNoH;
  double e2 = 0.0;
  for (int i = w.lane; i < s.n; i += W::kLanes) {
    double X, Y, x, y;
    if (!pt(i, &X, &Y, &x, &y)) continue;
    const double hw = H[6] * X + H[7] * Y + H[8];
    const double ex = (H[0] * X + H[1] * Y + H[2]) / hw - x, ey = (H[3] * X + H[4] * Y + H[5]) / hw - y;
    e2 += ex * ex + ey * ey;
  }
  const double fit = sqrt(w.allsum(e2) / m);
  if (max_fit_px > 0.0 && !(fit <= max_fit_px)) return kFocalBadFit;
  const double g = sqrt(2.0 / (H[0] * H[0] + H[3] * H[3] + H[1] * H[1] + H[4] * H[4]));
  if (!seed_finite(g * hsum)) return kFocalNoH;
  for (int k = 0; k < 9; ++k) o->H[k] = H[k] * g;
  const double h1x = o->H[0], h1y = o->H[3], h1z = o->H[6], h2x = o->H[1], h2y = o->H[4], h2z = o->H[7];
  const double c1 = h1x * h2x + h1y * h2y, d1 = -h1z * h2z;
  const double c2 = (h1x * h1x + h1y * h1y) - (h2x * h2x + h2y * h2y), d2 = h2z * h2z - h1z * h1z;
  o->rows[0] = c1; o->rows[1] = d1; o->rows[2] = c2; o->rows[3] = d2;
  const double cc = c1 * c1 + c2 * c2, q = (c1 * d1 + c2 * d2) / cc;
  o->f = (q > 0.0 && cc >= sin4) ? 1.0 / sqrt(q) : __builtin_nan("");
  o->fit_px = fit; o->used = m;
  return kFocalOk;
}

// One camera: list holds its n_list views in view order; rows (x 4) and status are those of all views of the batch.
template <class W>
VC_HD int focal_cam(const W& w, int n_list, const int* list, const int* status, const double* rows, double sin4, double* f, int* n_used) {
  int cnt = 0;
  double scc = 0.0, scd = 0.0;
  for (int j = w.lane; j < n_list; j += W::kLanes) {
    const size_t v = (size_t)list[j];
    if (status[v] != kFocalOk) continue;
    const double c1 = rows[4 * v], d1 = rows[4 * v + 1], c2 = rows[4 * v + 2], d2 = rows[4 * v + 3];
    ++cnt; scc += c1 * c1 + c2 * c2; scd += c1 * d1 + c2 * d2;
  }
  cnt = w.allsum(cnt); scc = w.allsum(scc); scd = w.allsum(scd);
  *n_used = cnt;
  if (cnt == 0) return kFocalCamNoView;
  if (!(scc >= sin4)) return kFocalCamNoTilt;
  const double q = scd / scc;
  if (!(q > 0.0) || !seed_finite(q)) return kFocalCamNoFocal;
  *f = sqrt(scc / scd);
  return kFocalCamOk;
}

// ---- the host side of vc_seed_focal.hip --------------------------------------------------------------------------------------
// The arguments are those of vc_seed_focal_batch, already checked.  kernel_ms (nullable): the mean time of the two kernels over time_reps
// more runs on the same input, back to back between two events.
int seed_focal_run(int device, int n_views, const int* view_cam, int n_cams, const double* cam_pp, const double* cam_radius, const int* view_off,
                   const double* p_w, const double* p_c, int min_corners, double max_fit_px, double min_tilt_deg, double* view_H, double* view_rows,
                   double* view_f, double* view_fit_px, int* view_used, int* view_status, double* cam_f, int* cam_views, int* cam_status,
                   int time_reps = 0, double* kernel_ms = nullptr);
bool seed_focal_args_ok(int n_views, const int* view_cam, int n_cams, const double* cam_pp, const double* cam_radius, const int* view_off,
                        const double* p_w, const double* p_c, double max_fit_px, double min_tilt_deg, const double* view_rows, const double* view_f,
                        const double* view_fit_px, const int* view_used, const int* view_status, const double* cam_f, const int* cam_views,
                        const int* cam_status);

}  // namespace vc
