// vc_lm_rules.hpp -- the trust-region constants of every Levenberg-Marquardt loop of the project.  Plain C++: host harnesses include it too.
#pragma once

namespace vc {

// The trust-region rules of the Levenberg-Marquardt loop (the Ceres rules the project restates), stated once: read by
// init_ctrl (vc_calibrator.hpp), lm_decide_local (vck_decide.hpp), the held-out pose refit (k_validate_pose, vc_validate.hip) and the model
// conversion's host loop (cvt_levenberg_marquardt, vc_convert.hpp).
struct LmRules {
  static constexpr double kInitialRadius = 1e4;
  static constexpr double kInitialDecrease = 2.0;          // radius /= decrease_factor on a rejection; the factor doubles with every one
  static constexpr double kMinRelativeDecrease = 1e-3;     // step quality above this accepts
  static constexpr double kMaxRadius = 1e16, kMinRadius = 1e-32;
  static constexpr double kInvalidShrink = 0.5;            // a step without a factorisation or a model decrease: radius *= 0.5
  static constexpr int kMaxInvalid = 5;                    // ... so many in a row end the solve as a failure
  static constexpr double kCallbackGnorm = 1e-9;           // iteration callback (vicalibrator.h:690-721): stop if 0 < |g| < this
};

}  // namespace vc
