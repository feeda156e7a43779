"""The end-to-end case of -dot_bias_rounds (tests/test_dot_bias_cli_gpu.py): a `linear` camera (f = 420 px, 640 x 480) sees the 9 x 6 board of
tests/dot_images.py (30 mm pitch, dot radii 9.4 / 6.3 mm by a fixed pattern) in 20 views at tilts up to 0.6 rad and 0.35 to 0.55 m.  The
measurements are the exact centres of the dots' image ellipses (conic algebra, tests/dot_bias_ref.py: linear_ellipse_centre), without noise: what
a perfect detector would return, and not the projections of the dots' centres.

build() also runs the experiment with the numpy reference alone -- a scipy least-squares calibration (intrinsics and the 20 poses) on those
measurements, the bias predicted at its result by tests/dot_bias_ref.py and subtracted, a second calibration -- and asserts that one round
removes at least a factor of 100 of the largest error of fx, fy, cx, cy: the yardstick the command line's factor of 20 is a margin below."""
import functools

import numpy as np

import dot_bias_cases as dc
import dot_bias_ref as ref
from vicalib_amd import synth

K_TRUE = np.array([420.0, 420.0, 319.5, 239.5])
N_VIEWS = 20


def _project(K, rot, t, P):
    pc = P @ synth.so3_exp_matrix(rot).T + t
    return np.stack([K[0] * pc[:, 0] / pc[:, 2] + K[2], K[1] * pc[:, 1] / pc[:, 2] + K[3]], axis=-1)


def _residuals(x, P, meas):
    return np.concatenate([(_project(x[:4], x[4 + 6 * v:7 + 6 * v], x[7 + 6 * v:10 + 6 * v], P) - meas[v]).ravel() for v in range(N_VIEWS)])


def _calibrate(x0, P, meas):
    from scipy.optimize import least_squares
    return least_squares(_residuals, x0, args=(P, meas), method="lm", xtol=1e-15, ftol=1e-15, gtol=1e-15, x_scale=np.concatenate([[100.0] * 4, np.tile([0.1] * 6, N_VIEWS)])).x


def _biases(x, P, radius):
    K = np.zeros(10); K[:4] = x[:4]
    out = np.zeros((N_VIEWS, len(P), 2))
    for v in range(N_VIEWS):
        T = dc.pose(x[4 + 6 * v:7 + 6 * v], x[7 + 6 * v:10 + 6 * v])
        for i in range(len(P)):
            st, b, _ = ref.one(ref.LINEAR, K, T, P[i], radius[i])
            assert st == ref.OK
            out[v, i] = b
    return out


@functools.lru_cache(maxsize=None)
def build():
    """dict: P [54, 3] (dot j * 9 + i at (i, j) * pitch), radius [54], pattern [6, 9] (1 = large), meas [20, 54, 2], K_true, and the reference's own
    experiment: err0, err1 (largest error of fx, fy, cx, cy without and with one round), rmse0, rmse1"""
    rng = np.random.default_rng(2024)
    ii, jj = np.meshgrid(np.arange(dc.NX), np.arange(dc.NY), indexing="xy")
    P = np.stack([ii.ravel() * dc.PITCH, jj.ravel() * dc.PITCH, np.zeros(dc.NX * dc.NY)], axis=-1)
    pattern = (rng.random((dc.NY, dc.NX)) < 0.4).astype(np.int32)
    radius = np.where(pattern.ravel() == 1, dc.R_LARGE, dc.R_SMALL)
    centre = np.array([0.5 * (dc.NX - 1) * dc.PITCH, 0.5 * (dc.NY - 1) * dc.PITCH, 0.0])
    x_true, meas = [K_TRUE], np.zeros((N_VIEWS, len(P), 2))
    for v in range(N_VIEWS):
        axis = np.append(rng.standard_normal(2), 0.3 * rng.standard_normal())
        rot = axis / np.linalg.norm(axis) * rng.uniform(0.1, 0.6)
        t = -synth.so3_exp_matrix(rot) @ centre + np.array([rng.uniform(-0.03, 0.03), rng.uniform(-0.02, 0.02), rng.uniform(0.35, 0.55)])
        x_true += [rot, t]
        T = dc.pose(rot, t)
        meas[v] = [ref.linear_ellipse_centre(K_TRUE, T, P[i], radius[i]) for i in range(len(P))]
        assert meas[v].min() > 5.0 and (meas[v] < np.array([635.0, 475.0])).all(), (v, meas[v].min(axis=0), meas[v].max(axis=0))
    x_true = np.concatenate(x_true)
    bias_true = meas - np.array([_project(K_TRUE, x_true[4 + 6 * v:7 + 6 * v], x_true[7 + 6 * v:10 + 6 * v], P) for v in range(N_VIEWS)])
    x0 = _calibrate(x_true, P, meas)
    corrected = meas - _biases(x0, P, radius)
    x1 = _calibrate(x0, P, corrected)
    err0, err1 = float(np.abs(x0[:4] - K_TRUE).max()), float(np.abs(x1[:4] - K_TRUE).max())
    rmse = lambda x, m: float(np.sqrt(np.mean(_residuals(x, P, m) ** 2)))
    out = dict(P=P, radius=radius, pattern=pattern, meas=meas, K_true=K_TRUE, err0=err0, err1=err1, rmse0=rmse(x0, meas), rmse1=rmse(x1, corrected),
               bias_rms=float(np.sqrt(np.mean(np.sum(bias_true ** 2, axis=-1)))), bias_max=float(np.sqrt(np.sum(bias_true ** 2, axis=-1)).max()))
    print("reference experiment: bias %.4f px rms, %.4f px max; error of fx fy cx cy %.3e px -> %.3e px (ratio %.0f); rmse %.3e -> %.3e px"
          % (out["bias_rms"], out["bias_max"], err0, err1, err0 / err1, out["rmse0"], out["rmse1"]))
    assert err0 / err1 >= 100.0, (err0, err1)
    assert out["rmse1"] < out["rmse0"]
    return out


def write(directory):
    """the detections file (frame,dot_id,u,v,X,Y,Z) and the pattern file of the case; returns their paths"""
    import os
    c = build()
    det, pat = os.path.join(directory, "cam0.csv"), os.path.join(directory, "pattern.txt")
    with open(det, "w") as f:
        for v in range(N_VIEWS):
            for i in range(len(c["P"])):
                f.write("%d,%d,%.17g,%.17g,%.17g,%.17g,%.17g\n" % (v, i, c["meas"][v, i, 0], c["meas"][v, i, 1], c["P"][i, 0], c["P"][i, 1], c["P"][i, 2]))
    with open(pat, "w") as f:
        for row in c["pattern"]:
            f.write(" ".join(str(int(x)) for x in row) + "\n")
    return det, pat


if __name__ == "__main__":
    build()
