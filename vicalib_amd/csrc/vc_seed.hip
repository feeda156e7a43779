// vc_seed.hip -- poses of many views of the planar target at once (gfx950, wave64, fp64 throughout): vc_pnp_planar_batch, and through it the
// device seeding of vc_init_frame_poses_pnp and of the held-out frames (vc_set_pnp_device).  vc_seed.hpp has the arithmetic.
//
//  k_seed_pnp   one wavefront per view, four views per workgroup, NO BLOCK BARRIER and no LDS: a view of 4 corners and a robust view of 190
//               finish after very different amounts of work, and nothing is shared between the waves.  Lanes stride over the view's
//               corners for the unprojection (undist_unproject, kept in the caller-sized xy work array: a lane reads back what it wrote
//               itself), the DLT sums, the refinement sums and the consensus sweeps.  The 9 x 9 eigen-solve of a DLT has lane k own row k
//               of the matrix and of the eigenvectors in registers; a Jacobi rotation exchanges two rows by lane reads (seed_eig9).
//               In the robust branch lane = hypothesis for the four-point poses, 64 per round; then the wave walks the round's
//               hypotheses: the pose comes by lane reads, one sweep over the corners gives count and error sum.  The best POSE is kept,
//               not its mask; the two masks a view needs (the best hypothesis's, the re-vote's) live in 2 n bytes of the work array.
//               Every sum over the corners is the fixed-order xor butterfly (wave_allsum): no floating-point atomic, every branch
//               behind a sum is wave-uniform, and a view gives the same bits alone, among others and on a second run.
// No CPU fallback: without a device the entry point fails.
#include <hip/hip_runtime.h>
#include <cstring>
#include <vector>
#include "../../include/vicalib_amd.h"
#include "vc_kutil.hpp"
#include "vc_hostutil.hpp"
#include "vc_seed.hpp"

namespace {

struct SeedBatch {
  int n_views, its;
  double tol;
  const int* model;       // per view
  const double* K;        // per view x 10
  const int* off;         // n_views + 1
  const double* pw;       // total x 3
  const double* uv;       // total x 2
  double* xy;             // total x 2 work
  char* mask;             // total x 2 work (view v: 2 n_v bytes from 2 off[v])
  double* T;              // n_views x 7
  double* rms;
  int* n_in;
  char* inlier;           // total
  int* status;
};

// the view's 64 lanes (vc_seed.hpp: W)
struct SeedWave {
  static constexpr int kLanes = 64;
  int lane;
  __device__ __forceinline__ double allsum(double x) const { return vc::wave_allsum(x); }
  __device__ __forceinline__ int allsum(int x) const { return vc::wave_allsum(x); }
  __device__ __forceinline__ double bcast(double x, int j) const { return vc::readlane_f64(x, j); }
  __device__ __forceinline__ int bcast(int x, int j) const { return __builtin_amdgcn_readlane(x, j); }
};

__global__ __launch_bounds__(256) void k_seed_pnp(SeedBatch b) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int v = __builtin_amdgcn_readfirstlane(blockIdx.x * 4 + wave);      // (scalar: the view's model, intrinsics and pointers are loaded once per wave)
  if (v >= b.n_views) return;                                     // (a whole wave leaves: nothing in this kernel waits for another wave)
  const size_t o0 = (size_t)b.off[v];
  vc::SeedView s;
  s.model = b.model[v]; s.n = b.off[v + 1] - b.off[v];
#pragma unroll
  for (int k = 0; k < 10; ++k) s.K[k] = b.K[(size_t)v * 10 + k];
  vc::model_precompute(s.model, s.K, &s.pre);
  s.pw = b.pw + 3 * o0; s.uv = b.uv + 2 * o0; s.xy = b.xy + 2 * o0; s.z0 = 0.0;
  double T[7], rms = 0.0;
  int n_in = 0;
  const char* flags = nullptr;
  const int status = vc::seed_view(SeedWave{lane}, s, b.its, b.tol, b.mask + 2 * o0, T, &rms, &n_in, &flags);
  char* inl = b.inlier + o0;
  for (int i = lane; i < s.n; i += 64) inl[i] = status != vc::kSeedOk ? 0 : (flags ? flags[i] : 1);
  if (lane == 0) {
    b.status[v] = status;
    if (status == vc::kSeedOk) {
#pragma unroll
      for (int k = 0; k < 7; ++k) b.T[(size_t)v * 7 + k] = T[k];
      b.rms[v] = rms; b.n_in[v] = n_in;
    }
  }
}

}  // namespace

namespace vc {

bool seed_batch_args_ok(int n_views, const int* view_model, const double* view_K, const int* view_off, const double* p_w, const double* p_c,
                        int iterations, double tol_px, const double* T_cw, const double* rms, const int* n_inliers, const int* status) {
  if (n_views < 0 || !view_model || !view_K || !view_off || !p_w || !p_c || !T_cw || !rms || !n_inliers || !status) return false;
  if (iterations < 0 || !(tol_px >= 0.0) || view_off[0] < 0) return false;
  for (int v = 0; v < n_views; ++v)
    if (view_off[v + 1] < view_off[v] || model_nk(view_model[v]) < 0) return false;
  return true;
}

int seed_batch_run(int device, void* stream_, int n_views, const int* view_model, const double* view_K, const int* view_off, const double* p_w,
                   const double* p_c, int iterations, double tol_px, double* T_cw, double* rms, int* n_inliers, char* inlier, int* status, int time_reps,
                   double* kernel_ms) {
  if (kernel_ms) *kernel_ms = 0.0;
  if (vch::open_device(device) != VC_OK) return VC_ERR_NO_DEVICE;
  if (n_views == 0) return VC_OK;
  hipStream_t stream = (hipStream_t)stream_;
  const size_t total = (size_t)view_off[n_views], nv = (size_t)n_views;
  SeedBatch b;
  std::memset(&b, 0, sizeof(b));
  b.n_views = n_views; b.its = iterations; b.tol = tol_px;
  int *d_model = nullptr, *d_off = nullptr;
  double *d_K = nullptr, *d_pw = nullptr, *d_uv = nullptr;
  auto carve = [&](vch::Carver q) {
    d_model = q.take<int>(nv); d_K = q.take<double>(nv * 10); d_off = q.take<int>(nv + 1);
    d_pw = q.take<double>(3 * total + 1); d_uv = q.take<double>(2 * total + 1);
    b.xy = q.take<double>(2 * total + 1); b.mask = q.take<char>(2 * total + 1);
    b.T = q.take<double>(nv * 7); b.rms = q.take<double>(nv); b.n_in = q.take<int>(nv);
    b.inlier = q.take<char>(total + 1); b.status = q.take<int>(nv);
    return q.bytes();
  };
  unsigned char* d_buf = nullptr;
  if (hipMalloc((void**)&d_buf, carve(vch::Carver())) != hipSuccess) return VC_ERR_NO_DEVICE;
  carve(vch::Carver(d_buf));
  b.model = d_model; b.K = d_K; b.off = d_off; b.pw = d_pw; b.uv = d_uv;
  std::vector<double> h_T(nv * 7), h_rms(nv);
  std::vector<int> h_n(nv);
  auto up = [&](void* dst, const void* src, size_t bytes) { return bytes == 0 || hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, stream) == hipSuccess; };
  auto down = [&](void* dst, const void* src, size_t bytes) { return bytes == 0 || hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, stream) == hipSuccess; };
  bool ok = up(d_model, view_model, nv * 4) && up(d_K, view_K, nv * 80) && up(d_off, view_off, (nv + 1) * 4) && up(d_pw, p_w, total * 24) &&
            up(d_uv, p_c, total * 16);
  if (ok) {
    hipLaunchKernelGGL(k_seed_pnp, dim3((n_views + 3) / 4), dim3(256), 0, stream, b);
    ok = hipGetLastError() == hipSuccess && down(h_T.data(), b.T, nv * 56) && down(h_rms.data(), b.rms, nv * 8) && down(h_n.data(), b.n_in, nv * 4) &&
         down(status, b.status, nv * 4) && (!inlier || down(inlier + view_off[0], b.inlier + view_off[0], total - (size_t)view_off[0]));
  }
  ok = hipStreamSynchronize(stream) == hipSuccess && ok;
  if (ok && kernel_ms && time_reps > 0)                              // (the kernel again on the same input: it writes the same bits)
    ok = vch::time_back_to_back(stream, time_reps, [&]() { hipLaunchKernelGGL(k_seed_pnp, dim3((n_views + 3) / 4), dim3(256), 0, stream, b); }, kernel_ms) == VC_OK;
  (void)hipFree(d_buf);
  if (!ok) return VC_ERR_NO_DEVICE;
  for (size_t v = 0; v < nv; ++v) {                                // a refused view's outputs are the caller's, untouched
    if (status[v] != kSeedOk) continue;
    std::memcpy(T_cw + 7 * v, &h_T[7 * v], 56);
    rms[v] = h_rms[v]; n_inliers[v] = h_n[v];
  }
  return VC_OK;
}

}  // namespace vc

extern "C" int vc_pnp_planar_batch(int device, int n_views, const int* view_model, const double* view_K, const int* view_off, const double* p_w,
                                   const double* p_c, int iterations, double tol_px, double* T_cw, double* rms, int* n_inliers, char* inlier, int* status) {
  if (!vc::seed_batch_args_ok(n_views, view_model, view_K, view_off, p_w, p_c, iterations, tol_px, T_cw, rms, n_inliers, status)) return VC_ERR_BAD_ARG;
  return vc::seed_batch_run(device, nullptr, n_views, view_model, view_K, view_off, p_w, p_c, iterations, tol_px, T_cw, rms, n_inliers, inlier, status, 0, nullptr);
}

extern "C" int vc_time_pnp_planar_batch(int device, int n_views, const int* view_model, const double* view_K, const int* view_off, const double* p_w,
                                        const double* p_c, int iterations, double tol_px, int reps, double* kernel_ms) {
  if (reps < 1 || !kernel_ms || n_views < 1) return VC_ERR_BAD_ARG;
  std::vector<double> T(7 * (size_t)n_views), rms(n_views);
  std::vector<int> n_in(n_views), status(n_views);
  if (!vc::seed_batch_args_ok(n_views, view_model, view_K, view_off, p_w, p_c, iterations, tol_px, T.data(), rms.data(), n_in.data(), status.data())) return VC_ERR_BAD_ARG;
  return vc::seed_batch_run(device, nullptr, n_views, view_model, view_K, view_off, p_w, p_c, iterations, tol_px, T.data(), rms.data(), n_in.data(), nullptr,
                            status.data(), reps, kernel_ms);
}
