"""The reference LM step of tests/lm_step_ref.py, pinned without a GPU: against the oracle's own dense and block solves of the same damped
system, and -- through vco_lm_lambda and vco_apply_step -- against the first iteration of the oracle's solve_once."""
import numpy as np
import pytest

import oracle_lib as ol
import lm_step_ref as ref
from vicalib_amd import synth


def _vision(models, n_frames, seed):
    p = synth.generate(synth.Config(models=models, n_frames=n_frames, seed=seed))
    orc = ol.Oracle().load(p); orc.set_options(calibrate_imu=False)
    orc.prepare(vis_mult=1)
    return p, orc


def _vi(models, n_frames, seed):
    p = synth.generate(synth.Config(models=models, n_frames=n_frames, imu=True, seed=seed))
    gt = p.imu_gt
    orc = ol.Oracle().load(p, init=False); orc.set_options(calibrate_imu=True)
    b0 = np.concatenate([gt["bg"], gt["ba"]]) * 0.7; s0 = np.concatenate([gt["sg"], gt["sa"]]) * 1.005
    orc.set_flags(True, True, False, True); orc.set_imu_state(b0, s0, np.array([0.02, 0.01]), 0.0013)
    orc.prepare(vis_mult=1, imu_mult=1)
    orc.update_imu_weights()
    return p, orc


@pytest.mark.parametrize("kind,models,n_frames", [("vision", ("poly3",), 12), ("vision", ("fov", "kb4"), 20), ("vision", ("kb4",) * 3, 16),
                                                  ("vi", ("kb4",), 20), ("vi", ("fov", "kb4"), 17)])
@pytest.mark.parametrize("radius", [1e0, 1e4, 1e8])
def test_reference_step_matches_the_oracle_dense_and_block_solves(kind, models, n_frames, radius):
    _, orc = (_vision if kind == "vision" else _vi)(models, n_frames, 7)
    lin = orc.linearize()
    df = 9 if kind == "vi" else 6
    lam = orc.lm_lambda(radius)
    r = ref.reference_step(lin, lam, df)
    print(f"{kind} {models} n={n_frames} radius={radius:g}: kappa(M~)={r['kappa']:.3e} bound={r['rel']:.3e}")
    tol = max(1e-10, r["rel"])              # the oracle's solves are Cholesky factorisations: as accurate as the bound allows
    assert radius > 1 or r["rel"] <= 1e-10
    xn = ref.scaled_norm(r, r["dfv"], r["dsv"])
    assert xn > 0
    for dense in (True, False):
        dfv, dsv = orc.solve_normal(lam, dense=dense)
        err = ref.scaled_norm(r, dfv - r["dfv"], dsv - r["dsv"])
        assert err <= tol * xn, (dense, err / xn)
    # the system the reference solves is the oracle's: its residual in long double is at rounding level
    n = lin["A"].shape[0]
    x = ref._pack(r["dfv"], r["dsv"], n, df)
    res = (r["M"].astype(np.longdouble) @ x.astype(np.longdouble) + r["g"]).astype(np.float64)
    assert np.linalg.norm(res * r["scale"]) <= 1e-13 * np.linalg.norm(r["g"] * r["scale"])


@pytest.mark.parametrize("models", [("poly3",), ("fov", "kb4")])
def test_damping_and_step_update_reproduce_the_first_iteration_of_solve_once(models):
    """vco_lm_lambda + the reference solve + vco_apply_step at the initial radius 1e4 give the trial point of the oracle's first LM
    iteration: its cost equals the cost that iteration records (accepted, so the trace's row 1 holds the cost at the new state)."""
    _, orc = _vision(models, 14, 3)
    lin = orc.linearize()
    r = ref.reference_step(lin, orc.lm_lambda(1e4), 6)
    orc.apply_step(r["dfv"], r["dsv"])
    trial_cost = orc.evaluate_cost()
    p, _ = _vision(models, 14, 3)
    run = ol.Oracle().load(p); run.set_options(calibrate_imu=False, max_iters=1)      # (solve() adds the one residual copy itself)
    run.solve()
    tr = run.trace()
    assert tr[1, 8] == 1 and tr[1, 7] > 1e4                 # accepted, radius grown
    assert abs(tr[0, 1] - lin["cost"]) <= 1e-12 * lin["cost"]
    assert abs(tr[1, 1] - trial_cost) <= 1e-9 * trial_cost


@pytest.mark.parametrize("world,n_frames", [(3, 20), (2, 17), (8, 16)])
@pytest.mark.parametrize("radius", [1e0, 1e4])
def test_separator_reduced_solve_reproduces_the_dense_step(world, n_frames, radius):
    """The separator layout the sharded GPU test compares against (lm_step_ref.separator_frames / sharded_order): eliminating every
    non-separator frame of the oracle's linearisation, solving the reduced system on the shared parameters and the separators, and
    back-substituting gives the dense reference step.  A wrong permutation in the helper fails here, without a GPU."""
    _, orc = _vi(("kb4",), n_frames, 7)
    lin = orc.linearize()
    lam = orc.lm_lambda(radius)
    r = ref.reference_step(lin, lam, 9)
    seps = ref.separator_frames(n_frames, world)
    assert seps == {3: [6, 13], 2: [8], 8: [2, 4, 6, 8, 10, 12, 14]}[world]       # the first frame of ranks 1 .. P - 1
    n = lin["A"].shape[0]
    d = ref.sharded_step(lin, lam, 9, seps)
    want = ref._pack(r["dfv"], r["dsv"], n, 9)
    s = r["scale"]
    err = np.linalg.norm((d - want) / s) / np.linalg.norm(want / s)
    print(f"world {world}, {n_frames} frames, radius {radius:g}: error {err:.3e}, bound {r['rel']:.3e}")
    assert err <= 1e-12, err
    ds, ss = ref.to_sharded(r, seps)
    D0 = lin["Hss"].shape[0]
    assert ds.shape == (D0 + 9 * (world - 1),) and ss.shape == ds.shape
    np.testing.assert_array_equal(ds[:D0], r["dsv"])
    for k, f in enumerate(seps):
        np.testing.assert_array_equal(ds[D0 + 9 * k:D0 + 9 * k + 9], r["dfv"][f])
    # the reduced system itself: its solution is the step's reduced part, and it is symmetric
    interior, reduced = ref.sharded_order(n, D0, seps, 9)
    assert len(set(interior) | set(reduced)) == n * 9 + D0 and not set(interior) & set(reduced)
    H = ref.dense_hessian(lin, 9)
    S, br, _, _ = ref.sharded_schur(H + np.diag(ref._pack(lam[:n * 9], lam[n * 9:], n, 9)), -r["g"], interior, reduced)
    np.testing.assert_allclose(S, S.T, rtol=0, atol=1e-12 * np.abs(S).max())
    np.testing.assert_allclose(S @ ds, br, rtol=0, atol=1e-9 * np.abs(br).max())
    # independent of sharded_order: the inverse of a Schur complement is the matching block of the inverse of the whole matrix, so each
    # separator's 9 x 9 block of S^-1, at columns D0 + 9 k, is the block of frame f = seps[k] of (H + Lambda)^-1, indexed by frame
    Minv = np.linalg.inv(H + np.diag(ref._pack(lam[:n * 9], lam[n * 9:], n, 9)))
    Sinv = np.linalg.inv(S)
    tol = 1e-9 * np.abs(Minv).max()
    np.testing.assert_allclose(Sinv[:D0, :D0], Minv[n * 9:, n * 9:], rtol=0, atol=tol)
    for k, f in enumerate({3: [6, 13], 2: [8], 8: [2, 4, 6, 8, 10, 12, 14]}[world]):
        np.testing.assert_allclose(Sinv[D0 + 9 * k:D0 + 9 * k + 9, D0 + 9 * k:D0 + 9 * k + 9], Minv[9 * f:9 * f + 9, 9 * f:9 * f + 9], rtol=0, atol=tol)
        np.testing.assert_allclose(Sinv[:D0, D0 + 9 * k:D0 + 9 * k + 9], Minv[n * 9:, 9 * f:9 * f + 9], rtol=0, atol=tol)
    # ... and a frame that is not a separator is nowhere in S: its block of (H + Lambda)^-1 matches no separator block of S^-1
    f = {3: 5, 2: 7, 8: 3}[world]
    assert all(np.abs(Sinv[D0 + 9 * k:D0 + 9 * k + 9, D0 + 9 * k:D0 + 9 * k + 9] - Minv[9 * f:9 * f + 9, 9 * f:9 * f + 9]).max() > 100 * tol
               for k in range(world - 1))
