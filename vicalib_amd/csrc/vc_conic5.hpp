// vc_conic5.hpp -- the 5 x 5 solve of the dual-conic fit, shared by the dot detector (vc_detect.hip: k_det_fit) and the predicted centre bias of
// a dot (vc_dot_bias.hpp).  An edge line l = (a, b, c) is tangent to the conic with dual [[A, B/2, D/2], [B/2, C, E/2], [D/2, E/2, 1]] when
// K . theta = -c^2, K = (a^2, a b, b^2, a c, b c), theta = (A, B, C, D, E); the weighted normal equations are sum w K K^T theta = -sum w K c^2
// and the conic's centre is (theta_3, theta_4) / 2 (Ouellet & Hebert 2009).
#pragma once
#include "vc_math.hpp"

// the loops are unrolled on the device: every index is a compile-time constant there and the matrix stays in registers
#if defined(__HIPCC__)
#define VC_C5_UNROLL _Pragma("unroll")
#else
#define VC_C5_UNROLL
#endif

namespace vc {

// acc: the 15 sums of the upper triangle of sum w K K^T, row by row, then the 5 sums of -w K c^2.  Gaussian elimination with partial
// pivoting (a row swap is a select on the pivot's row, not an array indexed at run time); false and theta = 0 when a pivot is exactly zero.
VC_HD bool conic5_solve(const double* acc, double* th) {
  double M[5][6];
  int e = 0;
  VC_C5_UNROLL
  for (int i = 0; i < 5; ++i) {
    VC_C5_UNROLL
    for (int j = i; j < 5; ++j) { M[i][j] = acc[e]; M[j][i] = acc[e]; ++e; }
  }
  VC_C5_UNROLL
  for (int i = 0; i < 5; ++i) { M[i][5] = acc[15 + i]; th[i] = 0.0; }
  bool ok = true;
  VC_C5_UNROLL
  for (int c = 0; c < 5; ++c) {
    if (!ok) continue;
    int p = c;
    double best = fabs(M[c][c]), pivot = M[c][c];
    VC_C5_UNROLL
    for (int rr = c + 1; rr < 5; ++rr)
      if (fabs(M[rr][c]) > best) { best = fabs(M[rr][c]); pivot = M[rr][c]; p = rr; }
    if (pivot == 0.0) { ok = false; continue; }
    VC_C5_UNROLL
    for (int rr = c + 1; rr < 5; ++rr) {
      if (p != rr) continue;
      VC_C5_UNROLL
      for (int j = 0; j < 6; ++j) { const double t = M[rr][j]; M[rr][j] = M[c][j]; M[c][j] = t; }
    }
    VC_C5_UNROLL
    for (int rr = c + 1; rr < 5; ++rr) {
      const double f = M[rr][c] / M[c][c];
      VC_C5_UNROLL
      for (int j = c; j < 6; ++j) M[rr][j] -= f * M[c][j];
    }
  }
  if (!ok) return false;
  VC_C5_UNROLL
  for (int i = 4; i >= 0; --i) {
    double s = M[i][5];
    VC_C5_UNROLL
    for (int j = i + 1; j < 5; ++j) s -= M[i][j] * th[j];
    th[i] = s / M[i][i];
  }
  return true;
}

}  // namespace vc
