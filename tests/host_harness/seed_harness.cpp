// TEST INFRASTRUCTURE: the arithmetic of the batched planar PnP (vicalib_amd/csrc/vc_seed.hpp, VC_HD) compiled for the host, so that the CPU
// suite can hold it against pnp_planar / pnp_planar_ransac without a GPU.  The pick sequence, the four-point homography, the DLT sums, the
// eigen-solve, pose from homography, the refinement's step rules and the consensus vote are the very functions the kernel runs; what the kernel
// adds is the 64 lanes of a wavefront and the order of the sums over corners, which are plain loops in corner order here (SeedSerial: one lane).
#include <cmath>
#include <cstring>
#include <vector>
#include "../../vicalib_amd/csrc/vc_seed.hpp"

extern "C" {

// one view, serially: the status of vc_pnp_planar_batch; with a status other than 0 the outputs are left alone and inlier (nullable) gets 0
int seed_harness_view(int model, const double* K /* 10 */, int n, const double* pw, const double* uv, int its, double tol, double* T_cw, double* rms,
                      int* n_inliers, char* inlier) {
  std::vector<double> xy(2 * (size_t)(n > 0 ? n : 1));
  std::vector<char> mask(2 * (size_t)(n > 0 ? n : 1), 0);
  vc::SeedView s;
  s.model = model; s.n = n;
  for (int k = 0; k < 10; ++k) s.K[k] = K[k];
  vc::model_precompute(model, s.K, &s.pre);
  s.pw = pw; s.uv = uv; s.xy = xy.data(); s.z0 = 0.0;
  double T[7], r = 0.0;
  int n_in = 0;
  const char* flags = nullptr;
  const int status = vc::seed_view(vc::SeedSerial(), s, its, tol, mask.data(), T, &r, &n_in, &flags);
  if (status != vc::kSeedOk) {
    if (inlier && n > 0) std::memset(inlier, 0, (size_t)n);
    return status;
  }
  std::memcpy(T_cw, T, sizeof(T));
  *rms = r; *n_inliers = n_in;
  if (inlier) for (int i = 0; i < n; ++i) inlier[i] = flags ? flags[i] : 1;
  return status;
}

// the picks of the first `its` iterations of a view of n corners: its x 4
void seed_harness_picks(int n, int its, int* table) {
  vc::SeedSampler s;
  vc::seed_sampler_init(&s, n);
  for (int k = 0; k < its; ++k) vc::seed_pick4(&s, n, table + 4 * k, table + 4 * k + 1, table + 4 * k + 2, table + 4 * k + 3);
}

}  // extern "C"
