// Host build of the odd-even elimination order of a chain group (vicalib_amd/csrc/vc_chain_order.hpp) for tests/test_chain_order_cpu.py:
// the schedule itself, and a block elimination + back-substitution of a bordered block-tridiagonal system that follows it the way the
// device kernels do (a frame touches its two neighbours of elimination time and the border, nothing else).
#include <cmath>
#include <vector>
#include "../../vicalib_amd/csrc/vc_chain_order.hpp"
#include "../../vicalib_amd/csrc/vc_chain_plan.hpp"

using namespace vc;

namespace {
constexpr int B = 9;
struct Dense {
  int n; std::vector<double> a;
  double& operator()(int i, int j) { return a[(size_t)i * n + j]; }
};
// in-place Cholesky of the b x b block at (o, o); false if not positive definite
bool chol(Dense& M, int o, int b, std::vector<double>& L) {
  L.assign((size_t)b * b, 0.0);
  for (int j = 0; j < b; ++j) {
    double d = M(o + j, o + j);
    for (int k = 0; k < j; ++k) d -= L[j * b + k] * L[j * b + k];
    if (!(d > 0.0)) return false;
    L[j * b + j] = std::sqrt(d);
    for (int i = j + 1; i < b; ++i) {
      double s = M(o + i, o + j);
      for (int k = 0; k < j; ++k) s -= L[i * b + k] * L[j * b + k];
      L[i * b + j] = s / L[j * b + j];
    }
  }
  return true;
}
void fwd_solve(const std::vector<double>& L, int b, double* x) {      // L x' = x
  for (int i = 0; i < b; ++i) { double s = x[i]; for (int k = 0; k < i; ++k) s -= L[i * b + k] * x[k]; x[i] = s / L[i * b + i]; }
}
void bwd_solve(const std::vector<double>& L, int b, double* x) {      // L^T x' = x
  for (int i = b - 1; i >= 0; --i) { double s = x[i]; for (int k = i + 1; k < b; ++k) s -= L[k * b + i] * x[k]; x[i] = s / L[i * b + i]; }
}
}  // namespace

extern "C" {

int vc_oe_steps(int q) { return oe_steps(q); }
int vc_oe_last(int q) { return oe_last(q); }
void vc_oe_frame(int q, int has_left, int has_right, int i, int* out4) {
  const OeFrame f = oe_frame(q, has_left != 0, has_right != 0, i);
  out4[0] = f.step; out4[1] = f.left; out4[2] = f.right; out4[3] = f.wave;
}
// the plan's odd-even fields: out = { n_levels, oe_top, oe[0 .. 15], two[0 .. 15] }
void vc_oe_plan(int N, int D, int n_cams, int imu_on, int sharded, int odd_even, int* out34) {
  ChainSwitches sw; sw.odd_even = odd_even != 0;
  const ChainPlan p = plan_chain(N, D, n_cams, imu_on != 0, sharded != 0, sw);
  out34[0] = p.n_levels; out34[1] = p.oe_top;
  for (int l = 0; l < kChainMaxLevels; ++l) { out34[2 + l] = p.oe[l]; out34[2 + kChainMaxLevels + l] = p.two[l]; }
}
void vc_oe_consts(int* out5) { out5[0] = kOeLeftSep; out5[1] = kOeRightSep; out5[2] = kOeNobody; out5[3] = kOeWaves; out5[4] = kOeMaxQ; }

// A: (P 9 + nb)^2 row-major, unknowns [left separator (if has_left) | frames 1 .. t | right separator (if has_right) | border]; rhs likewise.
// Eliminates the frames in the schedule's order -- round by round; a frame's Schur update goes ONLY to its two neighbours of the schedule
// and the border --, solves what is left (separators + border) densely, back-substitutes the last round first.  x: the solution.
int vc_oe_solve(int t, int has_left, int has_right, int nb, const double* A, const double* rhs, double* x) {
  const int P = t + (has_left ? 1 : 0) + (has_right ? 1 : 0), n = P * B + nb;
  Dense M{n, std::vector<double>(A, A + (size_t)n * n)};
  std::vector<double> g(rhs, rhs + n);
  auto pos = [&](int nbr) { return nbr == kOeLeftSep ? 0 : nbr == kOeRightSep ? (P - 1) * B : (nbr - 1 + (has_left ? 1 : 0)) * B; };
  const int ob = P * B;
  struct Img { std::vector<double> L, Y, z, Xs, Xn; int left, right; };
  std::vector<Img> img(t + 1);
  const int K = oe_steps(t);
  for (int st = 1; st <= K; ++st)
    for (int i = 1; i <= t; ++i) {
      const OeFrame f = oe_frame(t, has_left != 0, has_right != 0, i);
      if (f.step != st) continue;
      Img& I = img[i];
      I.left = f.left; I.right = f.right;
      const int o = pos(i);
      if (!chol(M, o, B, I.L)) return -1;
      // the frame's image: solved columns of the border, the right-hand side and the two couplings
      const int ncol = nb + 1 + 2 * B;
      std::vector<double> cols((size_t)ncol * B, 0.0);      // column-major: column c at cols[c * B]
      for (int c = 0; c < nb; ++c) for (int k = 0; k < B; ++k) cols[(size_t)c * B + k] = M(o + k, ob + c);
      for (int k = 0; k < B; ++k) cols[(size_t)nb * B + k] = g[o + k];
      if (f.left != kOeNobody) for (int c = 0; c < B; ++c) for (int k = 0; k < B; ++k) cols[(size_t)(nb + 1 + c) * B + k] = M(o + k, pos(f.left) + c);
      if (f.right != kOeNobody) for (int c = 0; c < B; ++c) for (int k = 0; k < B; ++k) cols[(size_t)(nb + 1 + B + c) * B + k] = M(o + k, pos(f.right) + c);
      for (int c = 0; c < ncol; ++c) fwd_solve(I.L, B, &cols[(size_t)c * B]);
      // target index of every image column in the big system (-1: the right-hand side, -2: nobody)
      std::vector<int> tgt(ncol);
      for (int c = 0; c < nb; ++c) tgt[c] = ob + c;
      tgt[nb] = -1;
      for (int c = 0; c < B; ++c) { tgt[nb + 1 + c] = f.left != kOeNobody ? pos(f.left) + c : -2; tgt[nb + 1 + B + c] = f.right != kOeNobody ? pos(f.right) + c : -2; }
      for (int r = 0; r < ncol; ++r) {
        if (tgt[r] < 0) continue;
        for (int c = 0; c < ncol; ++c) {
          if (tgt[c] == -2) continue;
          double s = 0.0;
          for (int k = 0; k < B; ++k) s += cols[(size_t)r * B + k] * cols[(size_t)c * B + k];
          if (tgt[c] == -1) g[tgt[r]] -= s; else M(tgt[r], tgt[c]) -= s;
        }
      }
      I.Y.assign(cols.begin(), cols.begin() + (size_t)nb * B);
      I.z.assign(cols.begin() + (size_t)nb * B, cols.begin() + (size_t)(nb + 1) * B);
      I.Xs.assign(cols.begin() + (size_t)(nb + 1) * B, cols.begin() + (size_t)(nb + 1 + B) * B);
      I.Xn.assign(cols.begin() + (size_t)(nb + 1 + B) * B, cols.end());
      // the frame leaves the system: whatever still couples to it would be an error of the schedule -- it stays in M and shows in the result
      for (int j = 0; j < n; ++j) if (j < o || j >= o + B) {
        bool known = (j >= ob);
        if (f.left != kOeNobody && j >= pos(f.left) && j < pos(f.left) + B) known = true;
        if (f.right != kOeNobody && j >= pos(f.right) && j < pos(f.right) + B) known = true;
        if (known) for (int k = 0; k < B; ++k) { M(o + k, j) = 0.0; M(j, o + k) = 0.0; }
      }
    }
  // what is left: separators + border (and, were the schedule wrong, couplings to eliminated frames)
  std::vector<int> keep;
  if (has_left) for (int k = 0; k < B; ++k) keep.push_back(k);
  if (has_right) for (int k = 0; k < B; ++k) keep.push_back((P - 1) * B + k);
  for (int c = 0; c < nb; ++c) keep.push_back(ob + c);
  const int m = (int)keep.size();
  for (int i = 1; i <= t; ++i) for (int k = 0; k < B; ++k) for (int j : keep) if (M(pos(i) + k, j) != 0.0) return -2;      // a coupling nobody eliminated
  Dense R{m, std::vector<double>((size_t)m * m)};
  std::vector<double> xr(m);
  for (int i = 0; i < m; ++i) { xr[i] = g[keep[i]]; for (int j = 0; j < m; ++j) R(i, j) = M(keep[i], keep[j]); }
  std::vector<double> Lr;
  if (m > 0) { if (!chol(R, 0, m, Lr)) return -3; fwd_solve(Lr, m, xr.data()); bwd_solve(Lr, m, xr.data()); }
  std::vector<double> sol(n, 0.0);
  for (int i = 0; i < m; ++i) sol[keep[i]] = xr[i];
  for (int st = K; st >= 1; --st)
    for (int i = 1; i <= t; ++i) {
      const Img& I = img[i];
      if (oe_frame(t, has_left != 0, has_right != 0, i).step != st) continue;
      double y[B];
      for (int k = 0; k < B; ++k) {
        double s = I.z[k];
        for (int c = 0; c < nb; ++c) s -= I.Y[(size_t)c * B + k] * sol[ob + c];
        if (I.left != kOeNobody) for (int c = 0; c < B; ++c) s -= I.Xs[(size_t)c * B + k] * sol[pos(I.left) + c];
        if (I.right != kOeNobody) for (int c = 0; c < B; ++c) s -= I.Xn[(size_t)c * B + k] * sol[pos(I.right) + c];
        y[k] = s;
      }
      bwd_solve(I.L, B, y);
      for (int k = 0; k < B; ++k) sol[pos(i) + k] = y[k];
    }
  for (int i = 0; i < n; ++i) x[i] = sol[i];
  return 0;
}

}  // extern "C"
