#pragma once
// vc_report.hpp -- what the residual report's kernels (vc_report.hip) and its host side (vc_report.cpp) share: the view of the report's
// buffers that travels in the kernel arguments and the launchers (the binning of the error map: vc_report_bins.hpp).
#include "vc_device.h"
#include "vc_report_bins.hpp"

namespace vc {

constexpr int kReportMapChunks = 1024;      // partial maps of the first pass at most (summed in chunk order by the second)
constexpr int kReportImuCols = 18;         // per IMU block: 9 whitened residuals, then the 9 unwhitened ones
struct ReportDropped { int frame, cam, pid, index; };      // a corner the outlier stage dropped: no longer in DevView's corner arrays

struct ReportView {
  int cur, wcur;                   // accepted state buffer, weight buffer holding the current weight_sqrt_
  // ---- vision sweep --------------------------------------------------------------------------------
  double2* res;                    // every corner the caller added, in the caller's order: (ru, rv) in pixels
  const int* obs_index;            // n_obs: device corner -> caller's index
  double* view_sq;                 // n_tiles: sum |r|^2
  double* view_max;                // n_tiles: max |r|
  long long* view_worst;           // n_tiles: caller's index of the corner that has it (lowest index on ties; -1: none)
  int* view_marked;                // n_tiles: corners kept with one copy fewer (kObsOneLess)
  int n_dropped;
  const ReportDropped* dropped;    // n_dropped
  const double2* dropped_uv;       // n_dropped
  // ---- error map ---------------------------------------------------------------------------------
  int bins_x, bins_y, n_chunks, tiles_per_chunk;
  int width[kMaxCams], height[kMaxCams];
  double* map_part;                // n_chunks x n_cams x cells x 4
  double* map;                     // n_cams x cells x 4: count, sum ru, sum rv, sum |r|^2
  // ---- IMU sweep ---------------------------------------------------------------------------------
  int n_blocks;
  const double* delta_blk;         // the blocks' delta records at the accepted state (k_imu_block into the report's own buffer)
  const double* grav;              // ... and its gravity record
  double* imu_out;                 // n_blocks x kReportImuCols
  int* imu_flags;                  // n_blocks: bit 0 = empty IMU range
};

// all asynchronous on `s`
void launch_report_vision(const DevView& v, const ReportView& r, hipStream_t s);      // corners of the problem + the dropped ones + view rows
void launch_report_map(const DevView& v, const ReportView& r, hipStream_t s);         // needs launch_report_vision
void launch_report_imu(const DevView& v, const ReportView& r, hipStream_t s);         // needs the delta records

}  // namespace vc
