// TEST INFRASTRUCTURE: the arithmetic of the registration kernels (vicalib_amd/csrc/vc_register.hpp, VC_HD) compiled for the host, and a
// sequential scatter over the same functions, so that the CPU suite can hold depth test, counters, gather and the continuous face
// against the numpy reference without a GPU.  What the kernels add is indexing and the atomics.  One thread.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>
#include "../../vicalib_amd/csrc/vc_register.hpp"

namespace {
struct Ray { double r[3]; bool ok; };
struct Harness {
  vc::RegisterPlan p;
  std::vector<Ray> centre, lattice;
  std::vector<unsigned long long> keys;      // of the last image of the last depth test
};
Ray ray_at(const vc::RegisterPlan& p, double u, double v) {
  Ray a;
  a.ok = vc::reg_ray(p, u, v, a.r);
  return a;
}
unsigned value_at(const unsigned char* img, int pitch, int i, int j) {
  unsigned short v;
  std::memcpy(&v, img + (size_t)j * pitch + 2 * (size_t)i, 2);
  return v;
}
// the depth test of one image into h->keys; counters (8, nullable) are added to; returns the number of key updates tried (what the
// kernel issues as atomics)
long long scatter(Harness* h, const unsigned char* img, int pitch, long long* counters) {
  const vc::RegisterPlan& p = h->p;
  h->keys.assign((size_t)p.d.w * p.d.h, vc::kRegEmptyKey);
  long long landed = 0;
  for (int j = 0; j < p.s.h; ++j)
    for (int i = 0; i < p.s.w; ++i) {
      const int e = j * p.s.w + i;
      const Ray& c = h->centre[e];
      const Ray& a = h->lattice[(size_t)j * (p.s.w + 1) + i];
      const Ray& b = h->lattice[(size_t)(j + 1) * (p.s.w + 1) + i + 1];
      unsigned w;
      vc::RegRect r;
      const int code = vc::reg_candidate(p, value_at(img, pitch, i, j), c.r, c.ok, a.r, a.ok, b.r, b.ok, &w, &r);
      if (counters) ++counters[code];
      if (code != vc::kRegCandidates) continue;
      const unsigned long long key = vc::reg_key(w, (unsigned)e);
      for (int y = r.y0; y <= r.y1; ++y)
        for (int x = r.x0; x <= r.x1; ++x) {
          unsigned long long& k = h->keys[(size_t)y * p.d.w + x];
          if (key < k) k = key;
          ++landed;
        }
    }
  return landed;
}
}  // namespace

extern "C" {

// poses as vc_get_camera returns them (unit quaternions); the tables of rays are built here, as at vc_registrar_create
void* vrh_create(int model_s, const double* Ks, int nks, int ws, int hs, const double* Ts, int model_d, const double* Kd, int nkd, int wd, int hd, const double* Td,
                 double unit_src, double unit_dst, int kind, int splat, int with_tables) {
  double ts[7], td[7];
  if (!vc::pose_ok(Ts, ts) || !vc::pose_ok(Td, td) || !vc::reg_args_ok(unit_src, unit_dst, kind, splat)) return nullptr;
  Harness* h = new Harness;
  std::memset(&h->p, 0, sizeof(h->p));
  vc::reg_cam_fill(&h->p.s, model_s, Ks, nks, ws, hs);
  vc::reg_cam_fill(&h->p.d, model_d, Kd, nkd, wd, hd);
  vc::reg_relative_pose(ts, td, h->p.R, h->p.t);
  h->p.unit_src = unit_src; h->p.unit_dst = unit_dst; h->p.kind = kind; h->p.splat = splat;
  if (with_tables) {
    for (int j = 0; j < hs; ++j) for (int i = 0; i < ws; ++i) h->centre.push_back(ray_at(h->p, i, j));
    for (int j = 0; j <= hs; ++j) for (int i = 0; i <= ws; ++i) h->lattice.push_back(ray_at(h->p, i - 0.5, j - 0.5));
  }
  return h;
}
void vrh_destroy(void* h) { delete static_cast<Harness*>(h); }
void vrh_get(void* hv, double* R, double* t) {
  Harness* h = static_cast<Harness*>(hv);
  std::memcpy(R, h->p.R, 72); std::memcpy(t, h->p.t, 24);
}

// the layout of vc_register_depth; landed (nullable): n, the key updates tried per image
void vrh_depth(void* hv, int n, const unsigned char* src, int src_pitch, long long src_stride, unsigned char* dst, int dst_pitch, long long dst_stride, int* index,
               long long* counters, long long* landed) {
  Harness* h = static_cast<Harness*>(hv);
  const int wd = h->p.d.w, hd = h->p.d.h;
  for (int k = 0; k < n; ++k) {
    long long c[vc::kRegCounters] = {0, 0, 0, 0, 0, 0, 0, 0};
    const long long tried = scatter(h, src + (size_t)k * src_stride, src_pitch, c);
    if (landed) landed[k] = tried;
    for (int y = 0; y < hd; ++y)
      for (int x = 0; x < wd; ++x) {
        const unsigned long long key = h->keys[(size_t)y * wd + x];
        const unsigned short d = (unsigned short)vc::reg_key_depth(key);
        std::memcpy(dst + (size_t)k * dst_stride + (size_t)y * dst_pitch + 2 * (size_t)x, &d, 2);
        if (index) index[((size_t)k * hd + y) * wd + x] = vc::reg_key_index(key);
        if (key != vc::kRegEmptyKey) ++c[vc::kRegFilled];
      }
    if (counters) std::memcpy(counters + (size_t)k * vc::kRegCounters, c, sizeof(c));
  }
}

// the layout of vc_register_color; value (nullable): n x h_s x w_s doubles, the unrounded bilinear value of a visible pixel
void vrh_color(void* hv, int n, const unsigned char* depth, int depth_pitch, long long depth_stride, const unsigned char* color, int color_pitch, long long color_stride,
               double occl_tol, int fill, unsigned char* out, int out_pitch, long long out_stride, unsigned char* mask, double* value) {
  Harness* h = static_cast<Harness*>(hv);
  const vc::RegisterPlan& p = h->p;
  for (int k = 0; k < n; ++k) {
    const unsigned char* dimg = depth + (size_t)k * depth_stride;
    scatter(h, dimg, depth_pitch, nullptr);
    for (int j = 0; j < p.s.h; ++j)
      for (int i = 0; i < p.s.w; ++i) {
        const size_t e = (size_t)j * p.s.w + i;
        const Ray& c = h->centre[e];
        double x, y, wr, val = NAN;
        int pix;
        bool vis = vc::reg_gather_position(p, value_at(dimg, depth_pitch, i, j), c.r, c.ok, &x, &y, &pix, &wr) && vc::reg_visible(wr, h->keys[pix], occl_tol);
        int v = fill;
        if (vis) {
          val = vc::reg_bilinear(color + (size_t)k * color_stride, color_pitch, p.d.w, p.d.h, x, y);
          v = std::min(std::max((int)std::floor(val + 0.5), 0), 255);
        }
        out[(size_t)k * out_stride + (size_t)j * out_pitch + i] = (unsigned char)v;
        if (mask) mask[(size_t)k * p.s.w * p.s.h + e] = vis ? 1 : 0;
        if (value) value[(size_t)k * p.s.w * p.s.h + e] = val;
      }
  }
}

void vrh_points(void* hv, int n, const double* in, double* out, unsigned char* valid) {
  Harness* h = static_cast<Harness*>(hv);
  for (int k = 0; k < n; ++k) {
    double o[3];
    const bool ok = vc::reg_point(h->p, in[3 * k], in[3 * k + 1], in[3 * k + 2], o);
    for (int c = 0; c < 3; ++c) out[3 * k + c] = ok ? o[c] : NAN;
    valid[k] = ok ? 1 : 0;
  }
}

}  // extern "C"
