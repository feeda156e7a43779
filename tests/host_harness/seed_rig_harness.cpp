// TEST INFRASTRUCTURE: the arithmetic of the rig seed (vicalib_amd/csrc/vc_seed_rig.hpp, VC_HD) compiled for the host, so that the CPU suite
// can hold it against tests/seed_rig_ref.py without a GPU.  The candidate, the agreement test, the refit's terms, the spreads, the index of
// shared frames, the argument checks and the tree are the very functions the kernels and the library run; what the kernels add is the order
// of the sums, which are plain loops in frame order here.
// With -DSEED_RIG_HARNESS_MAIN the file is a program of its own that runs the entry point once on a small rig (the sanitizer build).
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>
#include "../../vicalib_amd/csrc/vc_seed_rig.hpp"

extern "C" {

// the largest rig, the most frames, the vote's tile, the doubles of a candidate
void seed_rig_harness_constants(int out[4]) {
  out[0] = vc::kSeedRigMaxCams; out[1] = vc::kSeedRigMaxFrames; out[2] = vc::kSeedRigTile; out[3] = vc::kSeedRigRec;
}

// -2 / -7 for what the library refuses as a bad argument / as unsupported; the outputs as vc_seed_rig writes them
int seed_rig_harness_run(int n_frames, int n_cams, const unsigned char* view_ok, const double* view_T_cw, double tol_deg, int min_support, double* pair_T_ab,
                         int* pair_shared, int* pair_support, int* pair_winner, double* pair_rms_deg, double* pair_rms_m, int* pair_status, double* cam_T_c0,
                         int* cam_parent, int* cam_status) {
  const bool outs = pair_T_ab && pair_shared && pair_support && pair_winner && pair_rms_deg && pair_rms_m && pair_status && cam_T_c0 && cam_parent && cam_status;
  const int rc = vc::srig_judge(n_frames, n_cams, view_ok, view_T_cw, tol_deg, min_support, outs);
  if (rc != 0) return rc;
  vc::SrigIndex ix;
  vc::srig_build_index(n_frames, n_cams, view_ok, &ix);
  const vc::SrigTol tol = vc::srig_tol(tol_deg);
  const int P = ix.n_pairs;
  std::vector<int> status((size_t)P + 1), supp((size_t)P + 1, 0);
  std::vector<double> Tab(7 * (size_t)P + 1, 0.0);
  for (int p = 0; p < P; ++p) {
    const int n = ix.n[p];
    pair_shared[p] = n;
    std::vector<double> X((size_t)n * vc::kSeedRigRec);
    for (int e = 0; e < n; ++e) {
      const size_t f = (size_t)ix.frame[(size_t)ix.off[p] + e];
      vc::srig_candidate(view_T_cw + (f * n_cams + ix.a[p]) * 7, view_T_cw + (f * n_cams + ix.b[p]) * 7, &X[(size_t)e * vc::kSeedRigRec]);
    }
    int best = -1, we = -1;
    for (int i = 0; i < n; ++i) {
      int count = 0;
      for (int j = 0; j < n; ++j) count += vc::srig_agree(&X[(size_t)i * vc::kSeedRigRec], &X[(size_t)j * vc::kSeedRigRec], tol.cos_half, tol.tol2) ? 1 : 0;
      if (count > best) { best = count; we = i; }
    }
    status[p] = n == 0 ? vc::kSeedRigNoShared : best < min_support ? vc::kSeedRigFewSupport : vc::kSeedRigOk;
    pair_status[p] = status[p];
    if (status[p] != vc::kSeedRigOk) continue;
    const double* W = &X[(size_t)we * vc::kSeedRigRec];
    double acc[7] = {0, 0, 0, 0, 0, 0, 0}, T[7], a2 = 0.0, d2 = 0.0;
    int cnt = 0;
    for (int e = 0; e < n; ++e)
      if (vc::srig_agree(W, &X[(size_t)e * vc::kSeedRigRec], tol.cos_half, tol.tol2)) { vc::srig_refit_term(W, &X[(size_t)e * vc::kSeedRigRec], acc); ++cnt; }
    vc::srig_refit_finish(acc, cnt, T);
    for (int e = 0; e < n; ++e)
      if (vc::srig_agree(W, &X[(size_t)e * vc::kSeedRigRec], tol.cos_half, tol.tol2)) vc::srig_spread_term(T, &X[(size_t)e * vc::kSeedRigRec], &a2, &d2);
    vc::srig_spread_finish(a2, d2, cnt, &pair_rms_deg[p], &pair_rms_m[p]);
    supp[p] = cnt;
    std::memcpy(&Tab[7 * (size_t)p], T, sizeof(T));
    std::memcpy(pair_T_ab + 7 * (size_t)p, T, sizeof(T));
    pair_support[p] = cnt; pair_winner[p] = ix.frame[(size_t)ix.off[p] + we];
  }
  double cam_T[7 * vc::kSeedRigMaxCams];
  vc::srig_tree(n_cams, status.data(), supp.data(), Tab.data(), cam_T, cam_parent, cam_status);
  for (int c = 0; c < n_cams; ++c)
    if (cam_status[c] == vc::kSeedRigReached) std::memcpy(cam_T_c0 + 7 * (size_t)c, cam_T + 7 * (size_t)c, 56);
  return 0;
}

}  // extern "C"

#ifdef SEED_RIG_HARNESS_MAIN
// three cameras 0.1 m apart along x, 70 frames; camera 2 misses every third frame and has NaN there; one view of camera 1 is turned by 90 degrees
int main() {
  const int nf = 70, nc = 3;
  std::vector<unsigned char> ok((size_t)nf * nc, 1);
  std::vector<double> T(7 * (size_t)nf * nc);
  for (int k = 0; k < nf; ++k) {
    const double w[3] = {0.3 * std::sin(0.7 * k), 0.25 * std::cos(0.4 * k), 0.1 * std::sin(0.2 * k)};
    double q[4];
    vc::so3_exp(w, q);
    for (int c = 0; c < nc; ++c) {
      double* o = &T[7 * ((size_t)k * nc + c)];
      std::memcpy(o, q, sizeof(q));
      o[4] = 0.05 * std::sin(0.3 * k) - 0.1 * c; o[5] = 0.04 * std::cos(0.5 * k); o[6] = 0.7 + 0.2 * std::sin(0.11 * k);
      if (c == 2 && k % 3 == 0) { ok[(size_t)k * nc + c] = 0; for (int j = 0; j < 7; ++j) o[j] = std::nan(""); }
    }
  }
  {
    double* o = &T[7 * ((size_t)5 * nc + 1)];
    const double h = std::sqrt(0.5), turn[4] = {0, 0, h, h};
    double q[4];
    vc::quat_mul(turn, o, q);
    std::memcpy(o, q, sizeof(q));
  }
  double pT[21], rd[3], rm[3], cT[21];
  int sh[3], su[3], wi[3], st[3], par[3], cs[3];
  const int rc = seed_rig_harness_run(nf, nc, ok.data(), T.data(), 3.0, 3, pT, sh, su, wi, rd, rm, st, cT, par, cs);
  const int rb = seed_rig_harness_run(nf, nc, ok.data(), T.data(), 90.0, 3, pT, sh, su, wi, rd, rm, st, cT, par, cs);
  const int r0 = seed_rig_harness_run(0, 1, ok.data(), T.data(), 3.0, 3, pT, sh, su, wi, rd, rm, st, cT, par, cs);
  std::printf("run %d: pair (0,1) support %d of %d, t %.4f %.4f %.4f; camera 2: parent %d, t %.4f; refusal %d; empty %d\n", rc, su[0], sh[0], pT[4], pT[5], pT[6], par[2],
              cT[18], rb, r0);
  const bool good = rc == 0 && su[0] == nf - 1 && std::fabs(pT[4] - 0.1) < 1e-12 && par[2] >= 0 && std::fabs(cT[18] + 0.2) < 1e-12 && rb == -2 && r0 == 0;
  return good ? 0 : 1;
}
#endif
