#pragma once
// vc_holdout_select.hpp -- which frames the command line's -holdout_every N keeps out of the calibration: of the frames that survive
// -frame_skip and -num_vicalib_frames, numbered 0, 1, 2, ... in input order, the last of every full group of N (N - 1, 2N - 1, ...).
// A trailing group of fewer than N frames is fitted whole.  Host arithmetic, shared by apps/vicalib.cpp and tests/host_harness.
namespace vc {

inline bool holdout_is_held(long long i, int every) { return every >= 2 && i >= 0 && (i % every) == every - 1; }
inline long long holdout_num_held(long long n, int every) { return (every >= 2 && n > 0) ? n / every : 0; }
// N = 1 would hold every frame out; fewer than 2 fitting frames leave nothing to calibrate from
inline bool holdout_every_ok(long long n, int every) { return every == 0 || (every >= 2 && n - holdout_num_held(n, every) >= 2); }

}  // namespace vc
