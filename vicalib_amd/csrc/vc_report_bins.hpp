#pragma once
// vc_report_bins.hpp -- the binning of the residual report's error maps.  No HIP header: tests/test_report_cpu.py compiles it for the host.
#include <cmath>

#ifndef VC_HD
#if defined(__HIPCC__)
#define VC_HD __host__ __device__ __forceinline__
#else
#define VC_HD inline
#endif
#endif

namespace vc {

// Cell of the error map along one axis: clamp(int(floor(x * bins / extent)), 0, bins - 1), these operations in this order (one rounded
// product, one rounded quotient), so that a host restatement bins identically.  The clamp is applied before the conversion: a pixel far
// outside the image, or a NaN, lands in an edge cell instead of overflowing the integer.
VC_HD int report_cell(double x, int bins, int extent) {
  double q = x * (double)bins;
  q = q / (double)extent;
  q = floor(q);
  if (!(q > 0.0)) q = 0.0;
  if (q > (double)(bins - 1)) q = (double)(bins - 1);
  return (int)q;
}

}  // namespace vc
