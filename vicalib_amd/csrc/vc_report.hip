// vc_report.hip -- the residual report's device sweeps (gfx950, wave64): on demand, at the accepted state, outside any solve.
//
//  k_report_vision    one wavefront per (frame, camera) tile: every corner's residual with the solver's own arithmetic
//                     (make_tile_xf, model_precompute, corner_residual<MODEL>), stored at the corner's place in the CALLER's order;
//                     per view sum |r|^2, max |r| and the corner that has it, corners kept with one copy fewer
//  k_report_dropped   the corners the outlier stage dropped (they left the device's corner arrays): one thread per corner
//  k_report_map_part  error map, first pass: workgroup (chunk of tiles, camera) fills a slab of cells in LDS in corner order -- every lane
//                     owns the cells congruent to it modulo 64, so no two lanes ever add to the same cell and the order of the additions
//                     is the corners' -- and stores it as one partial map
//  k_report_map_sum   ... second pass: the partial maps added in chunk order.  No floating-point atomic anywhere: two reports of the same
//                     state give the same bits
//  k_report_imu       two threads per IMU block: the residual's tail (imu_block_final_direction, values only) on the block's delta record,
//                     once with the block's weight_sqrt_ (what the cost sees) and once with the identity (the functor's own units).  The
//                     delta records are k_imu_block's, launched on the report's own buffers
#include <hip/hip_runtime.h>
#include "vc_math.hpp"
#include "vc_imu.hpp"
#include "vc_device.h"
#include "vc_kutil.hpp"
#include "vc_view.hpp"
#include "vc_report.hpp"

namespace vc {

// a corner of the problem's tile-sorted arrays: u16 point ids that carry the one-copy-fewer mark
struct ReportCorners {
  const DevView& v; const int* obs_index;
  __device__ __forceinline__ ViewCorner operator()(int i) const {
    const int id = v.obs_pt[i];
    return {v.obs_uv[i], v.points + 3 * (size_t)(id & kObsPointMask), obs_index[i], (id & kObsOneLess) != 0};
  }
};
__global__ __launch_bounds__(256) void k_report_vision(DevView v, ReportView rp) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int tile = blockIdx.x * 4 + wave;
  if (tile >= v.n_tiles) return;
  const int f = v.tile_frame[tile], c = v.tile_cam[tile];
  const int off = v.tile_off[tile], cnt = v.tile_off[tile + 1] - off;
  TileXf x;
  double K[10];
  view_setup(v.poses[rp.cur] + (size_t)f * kPoseStride, v.cams[rp.cur] + (size_t)c * kCamStride, &x, K);
  with_model(v.cd[c].model, [&](auto m) {
    const ViewStats s = view_residuals<decltype(m)::value>(x, K, ReportCorners{v, rp.obs_index}, off, cnt, lane, rp.res);
    if (lane == 0) { rp.view_sq[tile] = s.sq; rp.view_max[tile] = s.max; rp.view_worst[tile] = s.worst; rp.view_marked[tile] = s.marked; }
  });
}

__global__ __launch_bounds__(64) void k_report_dropped(DevView v, ReportView rp) {
  const int i = blockIdx.x * 64 + threadIdx.x;
  if (i >= rp.n_dropped) return;
  const ReportDropped m = rp.dropped[i];
  const double2 uv = rp.dropped_uv[i];
  TileXf x;
  double K[10];
  view_setup(v.poses[rp.cur] + (size_t)m.frame * kPoseStride, v.cams[rp.cur] + (size_t)m.cam * kCamStride, &x, K);
  double r[2];
  with_model(v.cd[m.cam].model, [&](auto mc) {
    ModelPre pre;
    model_precompute(decltype(mc)::value, K, &pre);
    corner_residual<decltype(mc)::value>(x, K, pre, v.points + 3 * (size_t)m.pid, uv.x, uv.y, r);
  });
  rp.res[m.index] = make_double2(r[0], r[1]);
}

// ------------------------------------------------------------------------------------------ error map
// LDS: the slab (cells x 4) | 64 x (ru, rv) | 64 cells.  One wavefront per workgroup.
__global__ __launch_bounds__(64) void k_report_map_part(DevView v, ReportView rp) {
  extern __shared__ double lds[];
  const int lane = threadIdx.x, chunk = blockIdx.x, c = blockIdx.y;
  const int cells = rp.bins_x * rp.bins_y;
  double* slab = lds;
  double* s_r = lds + (size_t)cells * 4;
  int* s_cell = reinterpret_cast<int*>(s_r + 128);
  for (int i = lane; i < cells * 4; i += 64) slab[i] = 0.0;
  wave_lds_sync();
  const int t0 = chunk * rp.tiles_per_chunk, t1 = min(t0 + rp.tiles_per_chunk, v.n_tiles);
  const int W = rp.width[c], H = rp.height[c];
  for (int t = t0; t < t1; ++t) {
    if (v.tile_cam[t] != c) continue;                          // (wave-uniform)
    const int off = v.tile_off[t], cnt = v.tile_off[t + 1] - off;
    for (int base = 0; base < cnt; base += 64) {
      const int d = base + lane, nb = min(64, cnt - base);
      if (d < cnt) {
        const double2 uv = v.obs_uv[off + d];
        const double2 r = rp.res[rp.obs_index[off + d]];
        s_cell[lane] = report_cell(uv.y, rp.bins_y, H) * rp.bins_x + report_cell(uv.x, rp.bins_x, W);
        s_r[2 * lane] = r.x; s_r[2 * lane + 1] = r.y;
      }
      wave_lds_sync();
      for (int i = 0; i < nb; ++i) {                           // corner order; a lane adds to its own cells only
        const int ce = s_cell[i];
        if ((ce & 63) == lane) {
          const double a = s_r[2 * i], b = s_r[2 * i + 1];
          slab[4 * ce] += 1.0; slab[4 * ce + 1] += a; slab[4 * ce + 2] += b; slab[4 * ce + 3] += view_sq(a, b);
        }
      }
      wave_lds_sync();
    }
  }
  double* out = rp.map_part + ((size_t)chunk * v.n_cams + c) * cells * 4;
  for (int i = lane; i < cells * 4; i += 64) out[i] = slab[i];
}
__global__ __launch_bounds__(256) void k_report_map_sum(DevView v, ReportView rp) {
  const int n = v.n_cams * rp.bins_x * rp.bins_y * 4;
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e >= n) return;
  double s = 0.0;
  for (int g = 0; g < rp.n_chunks; ++g) s += rp.map_part[(size_t)g * n + e];
  rp.map[e] = s;
}

// ------------------------------------------------------------------------------------------ IMU blocks
__global__ __launch_bounds__(64) void k_report_imu(DevView v, ReportView rp) {
  __shared__ double s_eye[81];
  for (int i = threadIdx.x; i < 81; i += 64) s_eye[i] = (i % 10 == 0) ? 1.0 : 0.0;
  __syncthreads();
  const int idx = blockIdx.x * 64 + threadIdx.x;
  const int s = idx >> 1, which = idx & 1;                     // block s couples frames s -> s + 1; 0: whitened, 1: unwhitened
  if (s >= rp.n_blocks) return;
  const int j = s + 1;
  const double* T2 = v.poses[rp.cur] + (size_t)j * kPoseStride;
  const double* T1 = v.poses[rp.cur] + (size_t)(j - 1) * kPoseStride;
  const double* v2 = v.vel[rp.cur] + (size_t)j * 4;
  const double* v1 = v.vel[rp.cur] + (size_t)(j - 1) * 4;
  const double* brec = rp.delta_blk + (size_t)s * kBlockDeltaStride;
  const bool valid = brec[10] >= 0.0;
  const double* wq = which ? s_eye : v.wsqrtb[rp.wcur] + (size_t)s * 81;
  double r[9], dr[9];
  imu_block_final_direction(valid, brec, wq, v.rotation_only, T2, T1, v2, v1, rp.grav + rp.cur * 16, -1, r, dr);
  double* out = rp.imu_out + (size_t)s * kReportImuCols + 9 * which;
#pragma unroll
  for (int k = 0; k < 9; ++k) out[k] = valid ? r[k] : 0.0;
  if (which == 0) rp.imu_flags[s] = valid ? 0 : 1;
}

// ------------------------------------------------------------------------------------------ launchers
void launch_report_vision(const DevView& v, const ReportView& r, hipStream_t s) {
  if (v.n_tiles > 0) hipLaunchKernelGGL(k_report_vision, dim3((v.n_tiles + 3) / 4), dim3(256), 0, s, v, r);
  if (r.n_dropped > 0) hipLaunchKernelGGL(k_report_dropped, dim3((r.n_dropped + 63) / 64), dim3(64), 0, s, v, r);
}
void launch_report_map(const DevView& v, const ReportView& r, hipStream_t s) {
  if (v.n_cams <= 0) return;
  const int cells = r.bins_x * r.bins_y;
  const size_t lds = ((size_t)cells * 4 + 128) * sizeof(double) + 64 * sizeof(int);
  hipLaunchKernelGGL(k_report_map_part, dim3(r.n_chunks, v.n_cams), dim3(64), lds, s, v, r);
  hipLaunchKernelGGL(k_report_map_sum, dim3((v.n_cams * cells * 4 + 255) / 256), dim3(256), 0, s, v, r);
}
void launch_report_imu(const DevView& v, const ReportView& r, hipStream_t s) {
  if (r.n_blocks > 0) hipLaunchKernelGGL(k_report_imu, dim3((2 * r.n_blocks + 63) / 64), dim3(64), 0, s, v, r);
}

}  // namespace vc
