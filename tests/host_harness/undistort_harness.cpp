// TEST INFRASTRUCTURE: the arithmetic of the undistortion kernels (vicalib_amd/csrc/vc_undistort.hpp, VC_HD) compiled for the host, so that
// the CPU suite can hold the map entries and the point inverse against the oracle without a GPU.  What the kernels add is indexing only.
#include <cmath>
#include <cstring>
#include "../../vicalib_amd/csrc/vc_undistort.hpp"

static void fill_plan(vc::UndistPlan* p, int model, const double* K, int nk, int src_w, int src_h, const double* dl, int dst_w, int dst_h, const double* R_ds) {
  std::memset(p, 0, sizeof(*p));
  p->model = model; p->src_w = src_w; p->src_h = src_h; p->dst_w = dst_w; p->dst_h = dst_h; p->map_pitch = dst_w;
  for (int k = 0; k < nk; ++k) p->K[k] = K[k];
  vc::model_precompute(model, p->K, &p->pre);
  for (int k = 0; k < 4; ++k) p->dl[k] = dl[k];
  for (int i = 0; i < 3; ++i) for (int j = 0; j < 3; ++j) p->R_sd[3 * i + j] = R_ds ? R_ds[3 * j + i] : (i == j ? 1.0 : 0.0);
}

extern "C" {

// map: dst_h x dst_w x 2 floats (NaN pair = no source pixel), as vc_undistort_get_map returns it
void vuh_map(int model, const double* K, int nk, int src_w, int src_h, const double* dl, int dst_w, int dst_h, const double* R_ds, float* map) {
  vc::UndistPlan p;
  fill_plan(&p, model, K, nk, src_w, src_h, dl, dst_w, dst_h, R_ds);
  for (int j = 0; j < dst_h; ++j)
    for (int i = 0; i < dst_w; ++i) {
      double x, y;
      const bool ok = vc::undist_map_entry(p, i, j, &x, &y);
      map[2 * ((size_t)j * dst_w + i)] = ok ? (float)x : NAN;
      map[2 * ((size_t)j * dst_w + i) + 1] = ok ? (float)y : NAN;
    }
}
void vuh_points(int model, const double* K, int nk, const double* dl, const double* R_ds, int n, const double* in, double* out, unsigned char* valid) {
  vc::UndistPlan p;
  fill_plan(&p, model, K, nk, 2, 2, dl, 2, 2, R_ds);
  for (int k = 0; k < n; ++k) {
    double a, b;
    const bool ok = vc::undist_point(p, in[2 * k], in[2 * k + 1], &a, &b);
    out[2 * k] = ok ? a : NAN; out[2 * k + 1] = ok ? b : NAN; valid[k] = ok ? 1 : 0;
  }
}

}  // extern "C"
