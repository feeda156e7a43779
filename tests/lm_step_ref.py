"""Reference LM step for tests/test_lm_step_*.py: the damped normal equations of one LM iteration, formed from the oracle's
linearisation, solved densely in float64 with iterative refinement (residual in np.longdouble), plus the error bound every comparison
with it uses.  TEST INFRASTRUCTURE ONLY.

Bound.  The step is compared in Jacobi-scaled coordinates (x~ = x / s, s_i = 1 / (1 + sqrt(H_ii)), the scaling the solver itself uses):
M~ = S (H + Lambda) S is the scaled damped matrix, and a backward-stable solve of M~ x~ = -S g leaves
    || x~_dev - x~_ref || <= C_BOUND(n) * eps * kappa(M~) * || x~_ref ||,    C_BOUND(n) = 16 sqrt(n),
n the number of unknowns that have equations (frames without observations are decoupled and step by exactly zero)."""
import os
import sys

import numpy as np

EPS = np.finfo(np.float64).eps


def c_bound(n):
    return 16.0 * np.sqrt(n)


def dense_hessian(lin, df):
    """Gauss-Newton Hessian of the oracle's linearisation: frames (df = 6 or 9 per frame, block tridiagonal) first, then the D shared
    parameters."""
    A = lin["A"]; Cc = lin["C"]; W = lin["W"]; Hss = lin["Hss"]; n = A.shape[0]; D = Hss.shape[0]
    H = np.zeros((n * df + D, n * df + D))
    for f in range(n):
        s = slice(f * df, (f + 1) * df)
        H[s, s] = A[f, :df, :df]
        if f + 1 < n:
            s1 = slice((f + 1) * df, (f + 2) * df)
            H[s, s1] = Cc[f, :df, :df]; H[s1, s] = Cc[f, :df, :df].T
        H[s, n * df:] = W[f, :df]; H[n * df:, s] = W[f, :df].T
    H[n * df:, n * df:] = Hss
    return H


def _pack(frame_part, shared_part, n, df):
    return np.concatenate([np.asarray(frame_part).reshape(n, 9)[:, :df].ravel(), shared_part])


def reference_step(lin, lam, df):
    """Solves (H + Lambda) d = -g (lam in the oracle's N*9 + D indexing).  Returns dict with the step (frames n x 9, shared D), the
    Jacobi scale of every unknown, the active mask, kappa(M~) and the bound's factor C_BOUND * eps * kappa."""
    n = lin["A"].shape[0]; D = lin["Hss"].shape[0]
    H = dense_hessian(lin, df)
    hd = np.diag(H).copy()
    lv = _pack(lam[:n * 9], lam[n * 9:], n, df)
    g = _pack(lin["gf"], lin["gs"], n, df)
    act = np.abs(H).sum(axis=1) > 0
    M = H + np.diag(lv)
    s = 1.0 / (1.0 + np.sqrt(hd))
    Ma = M[np.ix_(act, act)]; sa = s[act]; b = -g[act]
    Ms = Ma * sa[:, None] * sa[None, :]
    bs = b * sa
    L = np.linalg.cholesky(Ms)

    def solve(r):
        return np.linalg.solve(L.T, np.linalg.solve(L, r))
    x = solve(bs)
    Mq, bq = Ms.astype(np.longdouble), bs.astype(np.longdouble)
    for _ in range(2):
        r = bq - Mq @ x.astype(np.longdouble)
        x = x + solve(r.astype(np.float64))
    ev = np.linalg.eigvalsh(Ms)
    kappa = ev[-1] / ev[0]
    d = np.zeros(n * df + D); d[act] = x * sa
    xs = np.zeros(n * df + D); xs[act] = x
    dfv = np.zeros((n, 9)); dfv[:, :df] = d[:n * df].reshape(n, df)
    na = int(act.sum())
    return dict(dfv=dfv, dsv=d[n * df:], scale=s, scaled=xs, active=act, kappa=kappa, n=na, rel=c_bound(na) * EPS * kappa, df=df, M=M, g=g)


def scaled_norm(ref, frame_part, shared_part):
    """|| x / s || over the active unknowns of a step given in the solve_normal layout."""
    n = ref["dfv"].shape[0]
    x = _pack(frame_part, shared_part, n, ref["df"]) / ref["scale"]
    return float(np.linalg.norm(x[ref["active"]]))


if __name__ == "__main__":      # child-process entry of the GPU test: python lm_step_ref.py <case name> (environment switches set by the parent)
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    import test_lm_step_gpu as t
    t.check_case(t.CASES[sys.argv[1]], child=True)
    print("ok", sys.argv[1])
