// TEST INFRASTRUCTURE: the arithmetic of the stereo consistency check (vicalib_amd/csrc/vc_rectify.hpp, VC_HD) compiled for the host, so that
// the CPU suite can hold the rotations, the pair arithmetic and the rigid fit against numpy without a GPU.  What the kernel adds is the
// indexing and the order of the sums.
#include <cmath>
#include <cstring>
#include "../../vicalib_amd/csrc/vc_rectify.hpp"

static void fill_plan(vc::UndistPlan* p, int model, const double* K, int nk, const double* dl, const double* R_ds) {
  std::memset(p, 0, sizeof(*p));
  p->model = model; p->src_w = 2; p->src_h = 2; p->dst_w = 2; p->dst_h = 2; p->map_pitch = 2;
  for (int k = 0; k < nk; ++k) p->K[k] = K[k];
  vc::model_precompute(model, p->K, &p->pre);
  for (int k = 0; k < 4; ++k) p->dl[k] = dl[k];
  for (int i = 0; i < 3; ++i) for (int j = 0; j < 3; ++j) p->R_sd[3 * i + j] = R_ds[3 * j + i];
}

extern "C" {

int vrh_rotations(const double* T_ck_a, const double* T_ck_b, double* R_ds_a, double* R_ds_b, double* baseline) {
  return vc::rectify_rotations(T_ck_a, T_ck_b, R_ds_a, R_ds_b, baseline);
}
// the rotation of the rigid fit from H = sum (P - Pm)(X - Xm)^T (row-major)
void vrh_rigid_rotation(const double* H, double* R) { vc::rigid_rotation(H, R); }

// the whole check of vc_rectify_check, frame by frame in plain loops: pairs n x 6, flags n, stats n_frames x 8 (count, invalid, sum dv,
// sum dv^2, max |dv|, worst, mean Z, rigid rms)
void vrh_check(int model_a, const double* Ka, int nka, const double* R_ds_a, int model_b, const double* Kb, int nkb, const double* R_ds_b, const double* dl,
               double baseline, int n_frames, const long long* frame_off, const double* px_a, const double* px_b, const double* target, double* pairs,
               unsigned char* flags, double* stats) {
  vc::RectPlan r;
  fill_plan(&r.a, model_a, Ka, nka, dl, R_ds_a); fill_plan(&r.b, model_b, Kb, nkb, dl, R_ds_b);
  r.baseline = baseline;
  for (int f = 0; f < n_frames; ++f) {
    int nv = 0;
    double s_dv = 0, s_dv2 = 0, s_z = 0, sp[3] = {0, 0, 0}, sx[3] = {0, 0, 0}, best = -1.0;
    long long best_i = -1;
    for (long long i = frame_off[f]; i < frame_off[f + 1]; ++i) {
      double o[6] = {NAN, NAN, NAN, NAN, NAN, NAN};
      const bool ok = vc::rectify_pair(r, px_a[2 * i], px_a[2 * i + 1], px_b[2 * i], px_b[2 * i + 1], o);
      std::memcpy(pairs + 6 * i, o, 48);
      flags[i] = ok ? 0 : 1;
      if (!ok) continue;
      ++nv; s_dv += o[0]; s_dv2 += o[0] * o[0]; s_z += o[4];
      for (int k = 0; k < 3; ++k) { sp[k] += o[2 + k]; if (target) sx[k] += target[3 * i + k]; }
      if (std::fabs(o[0]) > best) { best = std::fabs(o[0]); best_i = i; }
    }
    double rms = NAN;
    if (target && nv >= 3) {
      double Pm[3], Xm[3], H[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0}, R[9], ss = 0;
      for (int k = 0; k < 3; ++k) { Pm[k] = sp[k] / nv; Xm[k] = sx[k] / nv; }
      for (long long i = frame_off[f]; i < frame_off[f + 1]; ++i) {
        if (flags[i]) continue;
        for (int a = 0; a < 3; ++a) for (int b = 0; b < 3; ++b) H[3 * a + b] += (pairs[6 * i + 2 + a] - Pm[a]) * (target[3 * i + b] - Xm[b]);
      }
      vc::rigid_rotation(H, R);
      for (long long i = frame_off[f]; i < frame_off[f + 1]; ++i)
        if (!flags[i]) ss += vc::rigid_residual_sq(R, pairs + 6 * i + 2, Pm, target + 3 * i, Xm);
      rms = std::sqrt(ss / nv);
    }
    double* s = stats + 8 * (size_t)f;
    s[0] = nv; s[1] = (double)(frame_off[f + 1] - frame_off[f] - nv); s[2] = s_dv; s[3] = s_dv2; s[4] = best_i >= 0 ? best : 0.0; s[5] = (double)best_i;
    s[6] = nv > 0 ? s_z / nv : 0.0; s[7] = rms;
  }
}

}  // extern "C"
