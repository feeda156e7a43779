#pragma once
// vc_validate.hpp -- what the held-out scoring's kernels (vc_validate.hip) and its host side (vc_validate.cpp) share: the view of the
// hold-out set's buffers that travels in the kernel arguments, the status codes and the launchers.
#include "vc_device.h"

namespace vc {

// status of a held-out frame (vc_holdout_frames)
enum HoldoutStatus {
  kHoConverged = 0,          // a tolerance was met (gradient, function or parameter)
  kHoMaxIters = 1,           // the iteration cap ended the refit: the pose is the last accepted one
  kHoUnderdetermined = 2,    // fewer than 4 corners over all views: not fitted, residuals at the seed
  kHoNoSeed = 3,             // no seed pose: nothing evaluated (rows are zero)
  kHoFailed = 4              // five steps in a row without a usable factorisation or model decrease: the pose is the last accepted one
};
constexpr int kHoldoutDefaultIters = 50, kHoldoutMaxIters = 200;

struct HoldoutView {
  int n_frames, n_tiles, n_cams, max_iters;
  double ftol, gtol, ptol;
  int model[kMaxCams];
  const double* cams;            // n_cams x kCamStride: the frozen cameras (T_ck, intrinsics)
  const double* points;          // the hold-out set's own table of target points, 3 per point
  const int* frame_tile_off;     // n_frames + 1: the tiles of frame f are [frame_tile_off[f], frame_tile_off[f + 1])
  const int* tile_frame;         // n_tiles
  const int* tile_cam;           // n_tiles
  const int* tile_off;           // n_tiles + 1: corners of tile t
  const double2* obs_uv;         // detected pixels, tile order
  const int* obs_pt;             // point ids, tile order
  const int* obs_index;          // tile order -> the caller's order
  const double* seeds;           // n_frames x kPoseStride
  const int* seed_ok;            // n_frames
  // ---- pose refit ---------------------------------------------------------------------------------
  double* pose;                  // n_frames x kPoseStride: refined T_wk (the seed where nothing was fitted)
  int* status;                   // n_frames: HoldoutStatus
  int* iters;                    // n_frames: LM iterations (steps tried)
  int* behind;                   // n_frames: corners at depth <= 0 at the returned pose (they entered no sum)
  double* cost;                  // 2 x n_frames: cost at the seed, then at the returned pose (1/2 sum rho)
  // ---- residual sweep -----------------------------------------------------------------------------
  double2* res;                  // every corner in the caller's order
  double* view_sq;               // n_tiles
  double* view_max;              // n_tiles
  long long* view_worst;         // n_tiles
};

// both asynchronous on `s`
void launch_validate_pose(const HoldoutView& h, hipStream_t s);
void launch_validate_residuals(const HoldoutView& h, hipStream_t s);      // needs launch_validate_pose

}  // namespace vc
