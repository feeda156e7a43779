// vc_validate.hip -- held-out scoring (gfx950, wave64, fp64 throughout): a calibration is judged on views it was not estimated from.
// A held-out frame has no pose in the problem, so its rig pose is refitted with the cameras frozen before a residual means anything.
//
//  k_validate_pose       one wavefront per held-out frame runs the whole pose-only Levenberg-Marquardt solve of that frame: no host
//                        round trip per iteration, and NO BLOCK BARRIER anywhere -- the four waves of a workgroup hold four frames
//                        that finish after different iteration counts; nothing is shared between them (no LDS at all).
//                        Linearisation: lanes stride over the corners of each of the frame's tiles with the solver's own arithmetic
//                        (make_tile_xf, model_precompute, project_any<true>, loss_soft_l1); the frame Jacobian is the
//                        [A | A x q] diag(-R_ck, R_ck) form of tile_to_frame_blocks, applied per corner, so the step is a se3_plus
//                        increment.  Every lane accumulates the 21 + 6 + 1 sums of J^T W J, J^T W r and the cost with
//                        W = rho'(|r|^2) of SoftLOne(0.5) -- the first-order robustification only: NO Triggs second-order correction
//                        (the gradient is exact, the Gauss-Newton matrix is not corrected; the optimum is the same).  The sums are
//                        reduced by an xor butterfly of shuffles: a fixed order, every lane ends with the same bits, no
//                        floating-point atomic -- two runs, and a frame alone or among others, give the same bits.
//                        Step: (H + D / radius) delta = -g with D = clamp(diag H) (lm_clamped_diag, no Jacobi scaling: six
//                        parameters of one pose), 6 x 6 Cholesky in registers, trial pose by se3_plus, trial cost by a second sweep
//                        (project_any<false>).  Accept / reject / radius: the rules of lm_decide_local (vck_decide.hpp), with
//                        the solver's own constants (LmRules, vc_device.h).  A corner at depth <= 0 at the iterate enters no sum of that
//                        sweep and is counted.
//  k_validate_residuals  one wavefront per held-out (frame, camera) tile at the refined poses, in the manner of k_report_vision:
//                        (ru, rv) per corner at its place in the caller's order, per view sum |r|^2 (no contraction), max |r| and
//                        the corner that has it.
#include <hip/hip_runtime.h>
#include "vc_math.hpp"
#include "vc_device.h"
#include "vc_kutil.hpp"
#include "vc_view.hpp"
#include "vc_validate.hpp"

namespace vc {

constexpr int kHoAcc = 28;      // 21 (upper triangle of J^T W J, row by row) + 6 (J^T W r) + 1 (sum rho)

// One tile's corners into the lane's sums.  JAC: the linearisation (acc[0..27]); otherwise the cost alone (acc[27]).
template <int MODEL, bool JAC>
__device__ __forceinline__ void validate_tile_body(const HoldoutView& h, const TileXf& x, const double* Rck, const double* K, int off, int cnt,
                                                   int lane, double* acc, int* behind) {
  ModelPre pre;
  model_precompute(MODEL, K, &pre);
  for (int d = lane; d < cnt; d += 64) {
    const double2 uv = h.obs_uv[off + d];
    const double* pw = h.points + 3 * (size_t)h.obs_pt[off + d];
    double pc[3], pix[2], A[6], B[20];
    tile_point(x, pw, pc);
    if (!(pc[2] > 0.0)) { *behind += 1; continue; }           // behind the camera at this iterate: no sum of this sweep
    project_any<JAC>(MODEL, pc, K, pre, pix, JAC ? A : nullptr, JAC ? B : nullptr);
    const double r0 = pix[0] - uv.x, r1 = pix[1] - uv.y;
    double rho, w;
    loss_soft_l1(r0 * r0 + r1 * r1, &rho, &w);
    acc[27] += rho;
    if (JAC) {
      const double q0 = pc[0] - x.tck[0], q1 = pc[1] - x.tck[1], q2 = pc[2] - x.tck[2];
      double J[12];
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        const double* a = A + 3 * i;
        const double v0 = a[1] * q2 - a[2] * q1, v1 = a[2] * q0 - a[0] * q2, v2 = a[0] * q1 - a[1] * q0;      // A x q
#pragma unroll
        for (int j = 0; j < 3; ++j) {
          J[6 * i + j] = -(a[0] * Rck[j] + a[1] * Rck[3 + j] + a[2] * Rck[6 + j]);
          J[6 * i + 3 + j] = v0 * Rck[j] + v1 * Rck[3 + j] + v2 * Rck[6 + j];
        }
      }
      int k = 0;
#pragma unroll
      for (int a = 0; a < 6; ++a) {
        const double wa0 = w * J[a], wa1 = w * J[6 + a];
#pragma unroll
        for (int b = a; b < 6; ++b) acc[k++] += wa0 * J[b] + wa1 * J[6 + b];
        acc[21 + a] += wa0 * r0 + wa1 * r1;
      }
    }
  }
}

// One sweep over the frame's tiles at pose T, reduced over the wave: JAC fills Hu (21), g (6); returns the cost 1/2 sum rho.
template <bool JAC>
__device__ __forceinline__ double validate_sweep(const HoldoutView& h, int t0, int t1, const double* T, int lane, double* Hu, double* g, int* behind_out) {
  double acc[kHoAcc];
#pragma unroll
  for (int i = 0; i < kHoAcc; ++i) acc[i] = 0.0;
  int behind = 0;
  for (int t = t0; t < t1; ++t) {
    const int c = h.tile_cam[t];
    const int off = h.tile_off[t], cnt = h.tile_off[t + 1] - off;
    const double* cam = h.cams + (size_t)c * kCamStride;
    TileXf x;
    double Rck[9], K[10];
    view_setup(T, cam, &x, K);
    quat_to_R(cam, Rck);
    with_model(h.model[c], [&](auto m) { validate_tile_body<decltype(m)::value, JAC>(h, x, Rck, K, off, cnt, lane, acc, &behind); });
  }
  if (JAC) {
#pragma unroll
    for (int i = 0; i < 21; ++i) Hu[i] = wave_allsum(acc[i]);
#pragma unroll
    for (int i = 0; i < 6; ++i) g[i] = wave_allsum(acc[21 + i]);
  }
  *behind_out = wave_allsum(behind);
  return 0.5 * wave_allsum(acc[27]);
}

__device__ __forceinline__ double max_abs6(const double* g) {
  double m = 0.0;
#pragma unroll
  for (int i = 0; i < 6; ++i) m = fmax(m, fabs(g[i]));
  return m;
}

__global__ __launch_bounds__(256) void k_validate_pose(HoldoutView h) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int f = blockIdx.x * 4 + wave;
  if (f >= h.n_frames) return;                                 // (a whole wave leaves: nothing in this kernel waits for another wave)
  double T[7];
#pragma unroll
  for (int i = 0; i < 7; ++i) T[i] = h.seeds[(size_t)f * kPoseStride + i];
  const int t0 = h.frame_tile_off[f], t1 = h.frame_tile_off[f + 1];
  const int total = h.tile_off[t1] - h.tile_off[t0];
  int status, iter = 0, behind = 0;
  double cost0 = 0.0, cost = 0.0;
  if (!h.seed_ok[f]) {
    status = kHoNoSeed;
  } else if (total < 4) {
    status = kHoUnderdetermined;
    cost0 = cost = validate_sweep<false>(h, t0, t1, T, lane, nullptr, nullptr, &behind);
  } else {
    // every quantity below is the same in all 64 lanes (the sweeps end in all-lane sums): the control flow is wave-uniform
    double Hu[21], g[6];
    double radius = LmRules::kInitialRadius, decrease = LmRules::kInitialDecrease;
    int invalid = 0;
    cost0 = cost = validate_sweep<true>(h, t0, t1, T, lane, Hu, g, &behind);
    status = kHoMaxIters;
    if (!(cost == cost) || fabs(cost) > 1e300) status = kHoFailed;             // a seed nothing can be evaluated at
    else if (max_abs6(g) <= h.gtol) status = kHoConverged;
    while (status == kHoMaxIters && iter < h.max_iters) {
      ++iter;
      // ---- (H + D / radius) delta = -g --------------------------------------------------------------------------
      double M[36], D[6], delta[6];
      {
        int k = 0;
#pragma unroll
        for (int a = 0; a < 6; ++a)
#pragma unroll
          for (int b = a; b < 6; ++b) { M[a * 6 + b] = Hu[k]; M[b * 6 + a] = Hu[k]; ++k; }
      }
      const double ir = 1.0 / radius;
#pragma unroll
      for (int a = 0; a < 6; ++a) { D[a] = lm_clamped_diag(M[a * 6 + a], 1.0) * ir; M[a * 6 + a] += D[a]; delta[a] = -g[a]; }
      const bool ok = chol_small<6>(M);
      double model_change = 0.0, step2 = 0.0;
      if (ok) {
        fwd_solve<6>(M, delta); bwd_solve<6>(M, delta);
        double gd = 0.0, dld = 0.0;
#pragma unroll
        for (int a = 0; a < 6; ++a) { gd += g[a] * delta[a]; dld += delta[a] * D[a] * delta[a]; step2 += delta[a] * delta[a]; }
        model_change = -0.5 * gd + 0.5 * dld;
      }
      if (!ok || !(model_change > 0.0)) {                        // (NaN fails the comparison too)
        if (++invalid >= LmRules::kMaxInvalid) { status = kHoFailed; break; }
        radius *= LmRules::kInvalidShrink;
        continue;
      }
      invalid = 0;
      double x2 = 0.0;
#pragma unroll
      for (int i = 0; i < 7; ++i) x2 += T[i] * T[i];
      if (sqrt(step2) <= h.ptol * (sqrt(x2) + h.ptol)) { status = kHoConverged; break; }
      // ---- trial pose, trial cost ----------------------------------------------------------------------------
      double Tn[7];
      se3_plus(T, delta, Tn);
      int behind_n = 0;
      const double cost_n = validate_sweep<false>(h, t0, t1, Tn, lane, nullptr, nullptr, &behind_n);
      const bool finite = (cost_n == cost_n) && fabs(cost_n) <= 1e300;
      const double change = cost - cost_n;
      if (finite && fabs(change) < h.ftol * cost) { status = kHoConverged; break; }
      const double quality = change / model_change;
      if (finite && quality > LmRules::kMinRelativeDecrease) {
#pragma unroll
        for (int i = 0; i < 7; ++i) T[i] = Tn[i];
        const double q = 2.0 * quality - 1.0;
        radius = fmin(LmRules::kMaxRadius, radius / fmax(1.0 / 3.0, 1.0 - q * q * q));
        decrease = LmRules::kInitialDecrease;
        cost = validate_sweep<true>(h, t0, t1, T, lane, Hu, g, &behind);      // (the cost of the linearisation point, as the solver keeps it)
        if (max_abs6(g) <= h.gtol) { status = kHoConverged; break; }
      } else {                                                   // rejected (a non-finite trial cost included): more damping
        radius = radius / decrease; decrease *= 2.0;
        if (radius < LmRules::kMinRadius) { status = kHoConverged; break; }
      }
    }
  }
  if (lane == 0) {
#pragma unroll
    for (int i = 0; i < 7; ++i) h.pose[(size_t)f * kPoseStride + i] = T[i];
    h.pose[(size_t)f * kPoseStride + 7] = 0.0;
    h.status[f] = status; h.iters[f] = iter; h.behind[f] = behind;
    h.cost[f] = cost0; h.cost[(size_t)h.n_frames + f] = cost;
  }
}

// ------------------------------------------------------------------------------------------ residual sweep
// a corner of the hold-out set's tile-sorted arrays: plain point ids, never marked
struct HoldoutCorners {
  const HoldoutView& h;
  __device__ __forceinline__ ViewCorner operator()(int i) const { return {h.obs_uv[i], h.points + 3 * (size_t)h.obs_pt[i], h.obs_index[i], false}; }
};
__global__ __launch_bounds__(256) void k_validate_residuals(HoldoutView h) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int tile = blockIdx.x * 4 + wave;
  if (tile >= h.n_tiles) return;
  const int f = h.tile_frame[tile], c = h.tile_cam[tile];
  const int off = h.tile_off[tile], cnt = h.tile_off[tile + 1] - off;
  if (h.status[f] == kHoNoSeed) {                              // no pose: nothing evaluated, the rows are zero
    for (int d = lane; d < cnt; d += 64) h.res[h.obs_index[off + d]] = make_double2(0.0, 0.0);
    if (lane == 0) { h.view_sq[tile] = 0.0; h.view_max[tile] = 0.0; h.view_worst[tile] = -1; }
    return;
  }
  TileXf x;
  double K[10];
  view_setup(h.pose + (size_t)f * kPoseStride, h.cams + (size_t)c * kCamStride, &x, K);
  with_model(h.model[c], [&](auto m) {
    const ViewStats s = view_residuals<decltype(m)::value>(x, K, HoldoutCorners{h}, off, cnt, lane, h.res);
    if (lane == 0) { h.view_sq[tile] = s.sq; h.view_max[tile] = s.max; h.view_worst[tile] = s.worst; }
  });
}

// ------------------------------------------------------------------------------------------ launchers
void launch_validate_pose(const HoldoutView& h, hipStream_t s) {
  if (h.n_frames > 0) hipLaunchKernelGGL(k_validate_pose, dim3((h.n_frames + 3) / 4), dim3(256), 0, s, h);
}
void launch_validate_residuals(const HoldoutView& h, hipStream_t s) {
  if (h.n_tiles > 0) hipLaunchKernelGGL(k_validate_residuals, dim3((h.n_tiles + 3) / 4), dim3(256), 0, s, h);
}

}  // namespace vc
