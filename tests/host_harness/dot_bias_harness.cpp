// TEST INFRASTRUCTURE: the arithmetic of the predicted centre bias of a dot (vicalib_amd/csrc/vc_dot_bias.hpp, VC_HD) compiled for the host, so that
// the CPU suite can hold it against tests/dot_bias_ref.py without a GPU.  The projections, the edge lines, the twenty products and the 5 x 5 solve
// (vc_conic5.hpp, the detector's) are the very functions the kernel runs; what the kernel adds is the 64 lanes of a wavefront and the order of
// the sums, which are plain loops in sample order here (SeedSerial: one lane).  The layout of the arguments and the rule that a refused
// observation keeps the caller's values are those of vc_dot_bias_batch.
// With -DDOT_BIAS_HARNESS_MAIN the file is a program of its own (a few observations of every model, the statuses among them) for a run under
// the host sanitizers: g++ -fsanitize=address,undefined -DDOT_BIAS_HARNESS_MAIN dot_bias_harness.cpp && ./a.out
#include <cmath>
#include <cstdio>
#include <vector>
#include "../../vicalib_amd/csrc/vc_dot_bias.hpp"

extern "C" int dot_bias_harness_batch(int n_views, const int* view_model, const double* view_K, const double* view_T_cw, const int* view_off, const double* p_w,
                                      const double* radius, double* bias, double* radius_px, int* status) {
  for (int v = 0; v < n_views; ++v) {
    vc::DotBiasView view;
    vc::dot_bias_view(view_model[v], view_K + 10 * (size_t)v, view_T_cw + 7 * (size_t)v, &view);
    for (int i = view_off[v]; i < view_off[v + 1]; ++i) {
      double b[2] = {0.0, 0.0}, s = 0.0;
      status[i] = vc::dot_bias_one(vc::SeedSerial(), view, p_w + 3 * (size_t)i, radius[i], b, &s);
      if (status[i] != vc::kDotBiasOk) continue;
      bias[2 * (size_t)i] = b[0]; bias[2 * (size_t)i + 1] = b[1]; radius_px[i] = s;
    }
  }
  return 0;
}

#if defined(DOT_BIAS_HARNESS_MAIN)
int main() {
  const double Ks[6][10] = {{420, 420, 320, 240, 0.9}, {420, 420, 320, 240, -0.2, 0.05}, {420, 420, 320, 240, -0.2, 0.05, -0.01}, {260, 260, 320, 240, 0.01, -0.002, 0.0005, -0.0001},
                            {420, 420, 320, 240}, {420, 420, 320, 240, 0.1, 0.02, 0.001, 0.3, 0.03, 0.002}};
  const double nan = std::nan("");
  const double poses[4][7] = {{0.5, -0.1, 0.05, 0.85, -0.1, -0.05, 0.4}, {0, 0, 0, 1, 0, 0, 0.4}, {0, 0, 0, 1, 0, 0, -0.4}, {nan, 0, 0, 1, 0, 0, 0.4}};
  std::vector<int> model, off(1, 0);
  std::vector<double> K, T, pw, radius;
  for (int m = 0; m < 6; ++m)
    for (int p = 0; p < 4; ++p) {
      model.push_back(m);
      K.insert(K.end(), Ks[m], Ks[m] + 10);
      double q[7];
      for (int k = 0; k < 7; ++k) q[k] = poses[p][k];
      const double n = std::sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
      for (int k = 0; k < 4; ++k) q[k] /= n;
      T.insert(T.end(), q, q + 7);
      for (int j = 0; j < 3; ++j) { pw.insert(pw.end(), {0.03 * j, 0.02 * j, 0.0}); radius.push_back(j == 2 ? 0.0 : 0.0094); }
      pw.insert(pw.end(), {0.0, 0.0, 0.0}); radius.push_back(0.6);       // a rim that reaches behind the camera
      off.push_back((int)radius.size());
    }
  std::vector<double> bias(2 * radius.size(), -7.0), rpx(radius.size(), -7.0);
  std::vector<int> status(radius.size(), -1);
  dot_bias_harness_batch((int)model.size(), model.data(), K.data(), T.data(), off.data(), pw.data(), radius.data(), bias.data(), rpx.data(), status.data());
  int by_status[5] = {0, 0, 0, 0, 0};
  for (size_t i = 0; i < status.size(); ++i) {
    if (status[i] < 0 || status[i] > 4) { std::printf("observation %zu: status %d\n", i, status[i]); return 1; }
    ++by_status[status[i]];
    if (status[i] != 0 && (bias[2 * i] != -7.0 || rpx[i] != -7.0)) { std::printf("observation %zu: refused, but written\n", i); return 1; }
  }
  std::printf("%zu observations: status 0 x %d, 1 x %d, 2 x %d, 3 x %d, 4 x %d\n", status.size(), by_status[0], by_status[1], by_status[2], by_status[3], by_status[4]);
  return by_status[0] > 0 && by_status[1] > 0 && by_status[2] > 0 ? 0 : 1;
}
#endif
