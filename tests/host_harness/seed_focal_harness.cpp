// TEST INFRASTRUCTURE: the arithmetic of the focal-length seed (vicalib_amd/csrc/vc_seed_focal.hpp, VC_HD) compiled for the host, so that the CPU
// suite can hold it against tests/seed_focal_ref.py without a GPU.  The corner test, the DLT sums, the eigen-solve, the transfer error, the
// rows and the camera's sums are the very functions the kernels run; what the kernels add is the 64 lanes of a wavefront and the order of
// the sums, which are plain loops in corner and view order here (SeedSerial: one lane).  The layout of the arguments and the rule that a
// refused view or camera keeps the caller's values are those of vc_seed_focal_batch.
#include <cmath>
#include <cstring>
#include <vector>
#include "../../vicalib_amd/csrc/vc_seed_focal.hpp"

extern "C" int seed_focal_harness_batch(int n_views, const int* view_cam, int n_cams, const double* cam_pp, const double* cam_radius, const int* view_off,
                                        const double* p_w, const double* p_c, int min_corners, double max_fit_px, double min_tilt_deg, double* view_H,
                                        double* view_rows, double* view_f, double* view_fit_px, int* view_used, int* view_status, double* cam_f,
                                        int* cam_views, int* cam_status) {
  const double sin4 = vc::focal_sin4(min_tilt_deg);
  std::vector<double> rows(4 * (size_t)(n_views > 0 ? n_views : 1), 0.0);
  for (int v = 0; v < n_views; ++v) {
    const size_t o0 = (size_t)view_off[v];
    const int c = view_cam[v];
    vc::FocalView s;
    s.n = view_off[v + 1] - view_off[v]; s.pw = p_w + 3 * o0; s.uv = p_c + 2 * o0;
    s.cx = cam_pp[2 * c]; s.cy = cam_pp[2 * c + 1]; s.R = cam_radius[c];
    vc::FocalViewOut o;
    view_status[v] = vc::focal_view(vc::SeedSerial(), s, min_corners, max_fit_px, sin4, &o);
    if (view_status[v] != vc::kFocalOk) continue;
    if (view_H) std::memcpy(view_H + 9 * (size_t)v, o.H, sizeof(o.H));
    std::memcpy(view_rows + 4 * (size_t)v, o.rows, sizeof(o.rows));
    std::memcpy(&rows[4 * (size_t)v], o.rows, sizeof(o.rows));
    view_f[v] = o.f; view_fit_px[v] = o.fit_px; view_used[v] = o.used;
  }
  for (int c = 0; c < n_cams; ++c) {
    std::vector<int> list;
    for (int v = 0; v < n_views; ++v) if (view_cam[v] == c) list.push_back(v);
    double f = 0.0;
    cam_status[c] = vc::focal_cam(vc::SeedSerial(), (int)list.size(), list.data(), view_status, rows.data(), sin4, &f, &cam_views[c]);
    if (cam_status[c] == vc::kFocalCamOk) cam_f[c] = f;
  }
  return 0;
}
