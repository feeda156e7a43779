// vc_reg_rays.hpp -- the ray tables of a depth camera, shared by the kernel translation units that sweep its pixels (vc_register.hip,
// vc_depthcal.hip): the format, the load and the kernel that builds them.  A ray is an fp64 pair (x, y) plus z; z = NaN says that the
// position has no ray (vc::reg_ray: the Newton inversion failed, or r_z <= 0 under kind Z).
#pragma once
#include <hip/hip_runtime.h>
#include "vc_register.hpp"

namespace vc {

// centres [h_s][w_s]; lattice [h_s + 1][w_s + 1], node (i, j) at (i - 0.5, j - 0.5) (not built, and never read, without `lattice`)
struct RegTables {
  double2* c_xy; double* c_z;
  double2* l_xy; double* l_z;
};

__device__ __forceinline__ bool load_ray(const double2* xy, const double* z, size_t k, double* ray) {
  const double2 a = xy[k];
  ray[0] = a.x; ray[1] = a.y; ray[2] = z[k];
  return ray[2] == ray[2];
}

// one thread per entry: the centres first, then (lattice != 0) the nodes
static __global__ __launch_bounds__(256) void k_reg_rays(RegisterPlan p, RegTables t, int lattice) {
  const int ns = p.s.w * p.s.h, lw = p.s.w + 1, nl = lattice ? lw * (p.s.h + 1) : 0;
  const int k = blockIdx.x * 256 + threadIdx.x;
  if (k >= ns + nl) return;
  const bool centre = k < ns;
  const int e = centre ? k : k - ns, rw = centre ? p.s.w : lw;
  const int j = e / rw, i = e - j * rw;
  const double off = centre ? 0.0 : -0.5;
  double ray[3];
  const bool ok = reg_ray(p, (double)i + off, (double)j + off, ray);
  const double nan = __builtin_nan("");
  (centre ? t.c_xy : t.l_xy)[e] = ok ? make_double2(ray[0], ray[1]) : make_double2(nan, nan);
  (centre ? t.c_z : t.l_z)[e] = ok ? ray[2] : nan;
}

}  // namespace vc
