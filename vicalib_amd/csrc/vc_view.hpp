// vc_view.hpp -- the residual sweep over one (frame, camera) view, shared by the residual report (k_report_vision, vc_report.hip) and the
// held-out scoring (k_validate_residuals, vc_validate.hip).  The two differ only in where a corner comes from: `corner(i)` of the caller
// hands out corner i of the tile-sorted arrays as a ViewCorner.
#pragma once
#include "vc_math.hpp"
#include "vc_kutil.hpp"

namespace vc {

struct ViewCorner {
  double2 uv;            // detected pixel
  const double* pw;      // target point
  int index;             // the corner's place in the caller's order
  bool one_less;         // kept with one residual-block copy fewer (kObsOneLess)
};
struct ViewStats { double sq, max; long long worst; int marked; };      // sum |r|^2, max |r| (0: no corner), its corner (-1: none), one_less corners

// |r|^2 of the view rows and of the error map.  NOT cmp_norm2 (vc_compare.hpp): under hipcc __dmul_rn / __dadd_rn are plain * and +, which
// the compiler contracts to fma(rv, rv, ru * ru) -- one rounding fewer than the (ru * ru) + (rv * rv) a host restatement forms, a last-bit
// difference the tests allow for (1e-12).  Kept as it is: the unfused form would move bits of sum_sq, max_err and the map.
__device__ __forceinline__ double view_sq(double ru, double rv) { return __dadd_rn(__dmul_rn(ru, ru), __dmul_rn(rv, rv)); }

// One wavefront, the solver's own arithmetic (model_precompute, corner_residual<MODEL>): (ru, rv) of every corner stored at res[index]; the
// view's statistics in every lane.
template <int MODEL, class Corners>
__device__ __forceinline__ ViewStats view_residuals(const TileXf& x, const double* K, const Corners& corner, int off, int cnt, int lane, double2* res) {
  ModelPre pre;
  model_precompute(MODEL, K, &pre);
  double sq = 0.0, best = -1.0;
  long long best_i = -1;
  int marked = 0;
  for (int d = lane; d < cnt; d += 64) {                     // (ascending d = ascending caller index inside a view: ties keep the lowest)
    const ViewCorner c = corner(off + d);
    double r[2];
    corner_residual<MODEL>(x, K, pre, c.pw, c.uv.x, c.uv.y, r);
    res[c.index] = make_double2(r[0], r[1]);
    const double s2 = view_sq(r[0], r[1]);
    sq += s2;
    const double e = sqrt(s2);
    if (e > best) { best = e; best_i = c.index; }
    marked += c.one_less ? 1 : 0;
  }
  sq = wave_allsum(sq); marked = wave_allsum(marked);
  wave_argmax_low(&best, &best_i);
  return {sq, best_i >= 0 ? best : 0.0, best_i, marked};
}

}  // namespace vc
