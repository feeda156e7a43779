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


# ---- frame-sharded passes: the separator frames of the reduced system -------------------------------------------------------------

def separator_frames(n_frames, world):
    """Global index of the separator frames of a P-rank visual-inertial split, in column order: rank r > 0 moves its first frame
    (vicalib_amd.parallel.frame_shard) into the reduced system at columns D0 + 9 (r - 1) + [0, 9) (vc_upload.cpp: sep_col0), the 9
    in the frame's own order, pose 6 then velocity 3 (the back-substitution reads a pinned frame's step as delta_s[sep_col0 + i])."""
    from vicalib_amd.parallel import frame_shard
    return [frame_shard(n_frames, r, world)[0] for r in range(1, world)]


def sharded_order(n, D0, seps, df=9):
    """(interior, reduced): indices into the dense unknowns of dense_hessian (frames n * df, then the D0 shared parameters) of the
    frames a sharded pass eliminates, and of the D0 + df * len(seps) columns of its reduced system in their order."""
    sep_set = set(seps)
    interior = np.array([f * df + i for f in range(n) if f not in sep_set for i in range(df)], dtype=np.int64)
    reduced = np.array(list(range(n * df, n * df + D0)) + [f * df + i for f in seps for i in range(df)], dtype=np.int64)
    return interior, reduced


def sharded_schur(M, b, interior, reduced):
    """Dense Schur complement of M on the `reduced` unknowns: S = M_rr - M_ri M_ii^-1 M_ir, b_red = b_r - M_ri M_ii^-1 b_i.  Interior
    unknowns without equations (frames without detections, vision only) are decoupled and dropped."""
    act = np.abs(M[interior]).sum(axis=1) > 0
    i = interior[act]
    Mii = M[np.ix_(i, i)]; Mir = M[np.ix_(i, reduced)]
    X = np.linalg.solve(Mii, np.column_stack([Mir, b[i]]))
    k = len(reduced)
    return M[np.ix_(reduced, reduced)] - Mir.T @ X[:, :k], b[reduced] - Mir.T @ X[:, k], X, i


def sharded_step(lin, lam, df, seps):
    """The damped step solved the way a sharded pass solves it: eliminate every non-separator frame, solve the reduced system on the
    shared parameters and the separators, back-substitute.  Returns the step in the dense layout of dense_hessian."""
    n = lin["A"].shape[0]; D0 = lin["Hss"].shape[0]
    H = dense_hessian(lin, df)
    M = H + np.diag(_pack(lam[:n * 9], lam[n * 9:], n, df))
    g = _pack(lin["gf"], lin["gs"], n, df)
    interior, reduced = sharded_order(n, D0, seps, df)
    S, br, X, i = sharded_schur(M, -g, interior, reduced)
    Mii = M[np.ix_(i, i)]; Mir = M[np.ix_(i, reduced)]

    def solve(b):
        xi0 = np.linalg.solve(Mii, b[i])
        xr = np.linalg.solve(S, b[reduced] - Mir.T @ xi0)
        d = np.zeros(n * df + D0)
        d[reduced] = xr
        d[i] = xi0 - X[:, :-1] @ xr
        return d
    d = solve(-g)
    # one step of iterative refinement, residual in long double (as reference_step)
    res = (-g.astype(np.longdouble) - M.astype(np.longdouble) @ d.astype(np.longdouble)).astype(np.float64)
    return d + solve(res)


def device_columns(D0, n_seps, df):
    """Columns of the sharded reduced system that have a counterpart among the reference's unknowns, in the order of sharded_order: the
    shared D0, then the first df of each separator's 9 (pose 6, velocity 3).  With rotation-only initialisation the frames have df = 6
    unknowns; a separator keeps 9 columns, the last 3 without equations."""
    return np.array(list(range(D0)) + [D0 + 9 * j + i for j in range(n_seps) for i in range(df)], dtype=np.int64)


def to_sharded(ref, seps):
    """The reference step's delta_s and Jacobi scale in the sharded reduced system's column order (shared D0, then the separators)."""
    n, df = ref["dfv"].shape[0], ref["df"]
    D0 = len(ref["dsv"])
    _, reduced = sharded_order(n, D0, seps, df)
    d = _pack(ref["dfv"], ref["dsv"], n, df)
    return d[reduced], ref["scale"][reduced]


if __name__ == "__main__":      # child-process entry of the GPU test: python lm_step_ref.py <case name> (environment switches set by the parent)
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    import test_lm_step_gpu as t
    t.check_case(t.CASES[sys.argv[1]], child=True)
    print("ok", sys.argv[1])
