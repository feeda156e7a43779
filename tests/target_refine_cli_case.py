"""The end-to-end case of -refine_target_rounds (tests/test_target_refine_cli_gpu.py): a `linear` camera (f = 420 px, 640 x 480) sees a 9 x 6 board
(30 mm pitch) in 20 views at tilts of 0.1 to 0.6 rad and 0.35 to 0.55 m.  The board is not the grid: a 1.5 mm quadratic bow, x printed 0.2 % too
wide, a 0.3 mm in-plane wave -- every offset far below the default -refine_target_sigma of 10 mm.  The measurements are the exact projections of
the true board, without noise; the detections file names the NOMINAL grid.

build() also runs the experiment with the reference alone, at the command line's defaults (sigma = 0.01 m, two rounds): a scipy least-squares
calibration (intrinsics and the 20 poses) against the nominal grid, the numpy step of tests/target_refine_ref.py at its result, a calibration against
the refined target, and once more -- and asserts that the largest error of fx, fy, cx, cy falls by a factor of at least 100: the yardstick the
command line's factor of 20 is a margin below."""
import functools
import os

import numpy as np

import target_refine_ref as ref
from vicalib_amd import synth

K_TRUE = np.array([420.0, 420.0, 319.5, 239.5])
N_VIEWS, NX, NY, PITCH = 20, 9, 6, 0.03
SIGMA, ROUNDS = 0.01, 2


def _project(K, rot, t, P):
    pc = P @ synth.so3_exp_matrix(rot).T + t
    return np.stack([K[0] * pc[:, 0] / pc[:, 2] + K[2], K[1] * pc[:, 1] / pc[:, 2] + K[3]], axis=-1)


def _residuals(x, P, meas):
    return np.concatenate([(_project(x[:4], x[4 + 6 * v:7 + 6 * v], x[7 + 6 * v:10 + 6 * v], P) - meas[v]).ravel() for v in range(N_VIEWS)])


def _calibrate(x0, P, meas):
    from scipy.optimize import least_squares
    return least_squares(_residuals, x0, args=(P, meas), method="lm", xtol=1e-15, ftol=1e-15, gtol=1e-15, x_scale=np.concatenate([[100.0] * 4, np.tile([0.1] * 6, N_VIEWS)])).x


def _step(x, points, nominal, meas):
    """the reference's target step at the calibration x"""
    poses = []
    for v in range(N_VIEWS):
        R = synth.so3_exp_matrix(x[4 + 6 * v:7 + 6 * v])
        poses.append(synth.se3_from_Rt(R.T, -R.T @ x[7 + 6 * v:10 + 6 * v]))
    case = dict(cameras=[("linear", list(x[:4]), synth.se3_from_Rt(np.eye(3), np.zeros(3)), 4)], poses=np.array(poses),
                tiles=[(v, 0, np.arange(len(points)), meas[v]) for v in range(N_VIEWS)], points=points, nominal=nominal, lam=1.0 / SIGMA ** 2)
    r = ref.step(case)
    assert r["result_status"] == ref.OK and r["gauge_rank"] == 7
    return r["refined"]


def shape_error(target, true):
    """the largest distance between target and the true board after the best similarity (rotation, scale, translation) of target onto it, in metres"""
    a, b = target - target.mean(axis=0), true - true.mean(axis=0)
    U, S, Vt = np.linalg.svd(a.T @ b)
    D = np.diag([1.0, 1.0, np.sign(np.linalg.det(U @ Vt))])
    R = U @ D @ Vt
    scale = np.trace(np.diag(S) @ D) / np.sum(a * a)
    return float(np.sqrt(np.sum((scale * a @ R - b) ** 2, axis=1)).max())


@functools.lru_cache(maxsize=None)
def build():
    """dict: nominal [54, 3] (dot j * 9 + i at (i, j) * pitch), true [54, 3], meas [20, 54, 2], and the reference's own experiment: err (largest error of
    fx, fy, cx, cy without and after every round), rmse, shape (shape error of the nominal and of every round's target)"""
    rng = np.random.default_rng(2025)
    ii, jj = np.meshgrid(np.arange(NX), np.arange(NY), indexing="xy")
    nominal = np.stack([ii.ravel() * PITCH, jj.ravel() * PITCH, np.zeros(NX * NY)], axis=-1)
    centre = np.array([0.5 * (NX - 1) * PITCH, 0.5 * (NY - 1) * PITCH, 0.0])
    u = nominal - centre
    true = nominal + np.stack([0.002 * u[:, 0] + 3e-4 * np.sin(25.0 * u[:, 1]), 3e-4 * np.sin(20.0 * u[:, 0]), 1.5e-3 * ((u[:, 0] / 0.12) ** 2 + 0.5 * (u[:, 1] / 0.12) ** 2)], axis=1)
    assert np.abs(true - nominal).max() < 0.3 * SIGMA
    x_true, meas = [K_TRUE], np.zeros((N_VIEWS, len(nominal), 2))
    for v in range(N_VIEWS):
        axis = np.append(rng.standard_normal(2), 0.3 * rng.standard_normal())
        rot = axis / np.linalg.norm(axis) * rng.uniform(0.1, 0.6)
        t = -synth.so3_exp_matrix(rot) @ centre + np.array([rng.uniform(-0.03, 0.03), rng.uniform(-0.02, 0.02), rng.uniform(0.35, 0.55)])
        x_true += [rot, t]
        meas[v] = _project(K_TRUE, rot, t, true)
        assert meas[v].min() > 5.0 and (meas[v] < np.array([635.0, 475.0])).all(), (v, meas[v].min(axis=0), meas[v].max(axis=0))
    x = _calibrate(np.concatenate(x_true), nominal, meas)
    rmse = lambda x, P: float(np.sqrt(np.mean(_residuals(x, P, meas) ** 2)))
    points = nominal
    err, rm, shape = [float(np.abs(x[:4] - K_TRUE).max())], [rmse(x, points)], [shape_error(nominal, true)]
    for _ in range(ROUNDS):
        points = _step(x, points, nominal, meas)
        x = _calibrate(x, points, meas)
        err.append(float(np.abs(x[:4] - K_TRUE).max())); rm.append(rmse(x, points)); shape.append(shape_error(points, true))
    print("reference experiment at sigma %g m: error of fx fy cx cy %s px (ratio %.0f); rmse %s px; shape error %s mm"
          % (SIGMA, ", ".join("%.3e" % e for e in err), err[0] / err[-1], ", ".join("%.3e" % e for e in rm), ", ".join("%.5f" % (1e3 * e) for e in shape)))
    assert err[0] / err[-1] >= 100.0, err
    assert rm[-1] < rm[0]
    return dict(nominal=nominal, true=true, meas=meas, K_true=K_TRUE, err=err, rmse=rm, shape=shape)


def write(directory):
    """the detections file (frame,dot_id,u,v,X,Y,Z with the NOMINAL grid) of the case; returns its path"""
    c = build()
    det = os.path.join(directory, "cam0.csv")
    with open(det, "w") as f:
        for v in range(N_VIEWS):
            for i in range(len(c["nominal"])):
                f.write("%d,%d,%.17g,%.17g,%.17g,%.17g,%.17g\n" % (v, i, c["meas"][v, i, 0], c["meas"][v, i, 1], c["nominal"][i, 0], c["nominal"][i, 1], c["nominal"][i, 2]))
    return det


if __name__ == "__main__":
    build()
