"""Numpy restatement of the IMU noise characterisation (vicalib_amd/csrc/vc_allan.hpp): the overlapping Allan variance from prefix sums, the
averaging factors and their standard error, the static stretch, the fit of white noise, bias instability and rate random walk.
Every quantity has two routes, and the spread between them is the conditioning of a case: the prefix sums S accumulated in float64 and in
numpy.longdouble; the fit by its normal equations and by numpy.linalg.lstsq on the weighted system."""
import numpy as np

BIAS_FACTOR = 2.0 * np.log(2.0) / np.pi
CHANNELS = ("gx", "gy", "gz", "ax", "ay", "az")


def channels(gyro, accel):
    """n x 3, n x 3 -> 6 x n"""
    return np.ascontiguousarray(np.concatenate([np.asarray(gyro, dtype=np.float64).T, np.asarray(accel, dtype=np.float64).T]))


def prefix(y, dtype=np.float64):
    """S_0 = 0, S_k = sum_{i<k} (y_i - mean): n + 1 values in dtype"""
    y = np.asarray(y, dtype=dtype)
    return np.concatenate([np.zeros(1, dtype=dtype), np.cumsum(y - y.mean(dtype=dtype), dtype=dtype)])


def terms(count, m):
    return count - 2 * m + 1


def avar(y, ms, first=0, count=None, dtype=np.float64):
    """the overlapping Allan variance of the samples [first, first + count) of one channel at every factor of ms -> float64 [len(ms)]"""
    y = np.asarray(y, dtype=np.float64)[first:(None if count is None else first + count)]
    S = prefix(y, dtype)
    n = len(y)
    out = np.zeros(len(ms))
    for j, m in enumerate(ms):
        m = int(m)
        t = terms(n, m)
        assert m >= 1 and t >= 1, (n, m)
        d = S[2 * m:2 * m + t] - 2 * S[m:m + t] + S[:t]
        out[j] = np.float64(np.sum(d * d, dtype=dtype) / (dtype(2.0) * m * m * t))
    return out


def avar6(gyro, accel, ms, first=0, count=None, dtype=np.float64):
    return np.stack([avar(y, ms, first, count, dtype) for y in channels(gyro, accel)])


def rel_err(n_used, m):
    return 1.0 / np.sqrt(2.0 * (n_used / np.asarray(m, dtype=np.float64) - 1.0))


def factors(n_used, per_decade=20, max_fraction=1.0 / 9.0):
    m_max = max(1, int(np.floor(n_used * max_fraction)))
    out, j = [], 0
    while True:
        v = int(np.floor(10.0 ** (j / per_decade) + 0.5))
        if v > m_max:
            break
        if not out or v > out[-1]:
            out.append(v)
        j += 1
    return np.array(out, dtype=np.int32)


def log_info(time):
    """tau0, dt_min, dt_max, the intervals outside [0.5, 1.5] tau0"""
    t = np.asarray(time, dtype=np.float64)
    dt = np.diff(t)
    tau0 = (t[-1] - t[0]) / (len(t) - 1)
    return tau0, dt.min(), dt.max(), int(np.sum(~((dt >= 0.5 * tau0) & (dt <= 1.5 * tau0))))


# ---------------------------------------------------------------------------------------------- the static stretch
def window_change(gyro, accel, W, dtype=np.float64):
    """the statistic of every window start 0 .. n - 2W for both sensors -> float64 [2, n - 2W + 1]"""
    S = np.stack([prefix(y, dtype) for y in channels(gyro, accel)])
    n = S.shape[1] - 1
    t = n - 2 * W + 1
    d = (S[:, 2 * W:2 * W + t] - 2 * S[:, W:W + t] + S[:, :t]) / dtype(W)
    return np.stack([np.sqrt((d[:3] ** 2).sum(axis=0)), np.sqrt((d[3:] ** 2).sum(axis=0))]).astype(np.float64)


def static(gyro, accel, W, gyro_thr, accel_thr, dtype=np.float64):
    """-> (status, first, count, n_quiet); status 1 (first = count = None) when no start is quiet"""
    q = window_change(gyro, accel, W, dtype)
    quiet = np.ones(q.shape[1], dtype=bool)
    if gyro_thr > 0:
        quiet &= q[0] < gyro_thr
    if accel_thr > 0:
        quiet &= q[1] < accel_thr
    best, best_at, run = 0, 0, 0
    for k, v in enumerate(quiet):
        run = run + 1 if v else 0
        if run > best:
            best, best_at = run, k - run + 1
    if best == 0:
        return 1, None, None, 0
    return 0, best_at, best - 1 + 2 * W, int(quiet.sum())


# ---------------------------------------------------------------------------------------------- the fit
def basis(tau):
    tau = np.asarray(tau, dtype=np.float64)
    return np.stack([1.0 / tau, np.full_like(tau, BIAS_FACTOR), tau / 3.0], axis=1)


def model(N, B, K, tau):
    return basis(tau) @ np.array([N * N, B * B, K * K])


def fit(tau, av, e, route="normal"):
    """-> dict(N, B, K, mask, rms_log, status, n_points)"""
    tau, av, e = (np.asarray(a, dtype=np.float64) for a in (tau, av, e))
    ok = np.isfinite(tau) & np.isfinite(av) & np.isfinite(e) & (tau > 0) & (av > 0) & (e > 0)
    tau, av, e = tau[ok], av[ok], e[ok]
    out = dict(N=0.0, B=0.0, K=0.0, mask=0, rms_log=0.0, status=0, n_points=int(ok.sum()))
    if out["n_points"] < 3:
        out["status"] = 1
        return out
    A = basis(tau) / (av * e)[:, None]
    y = 1.0 / e
    best = None
    for mask in range(1, 8):
        idx = [a for a in range(3) if mask & (1 << a)]
        Am = A[:, idx]
        if route == "normal":
            s = np.sqrt((Am * Am).sum(axis=0))
            try:
                L = np.linalg.cholesky((Am / s).T @ (Am / s))
            except np.linalg.LinAlgError:
                continue
            x = np.linalg.solve(L.T, np.linalg.solve(L, (Am / s).T @ y)) / s
        else:
            x, _, rank, _ = np.linalg.lstsq(Am, y, rcond=None)
            if rank < len(idx):
                continue
        if not (np.all(np.isfinite(x)) and np.all(x >= 0)):
            continue
        res = float(((Am @ x - y) ** 2).sum())
        if best is None or res < best[0]:
            full = np.zeros(3)
            full[idx] = x
            best = (res, mask, full)
    if best is None:
        out["status"] = 2
        return out
    N, B, K = np.sqrt(best[2])
    out.update(N=N, B=B, K=K, mask=best[1], rms_log=float(np.sqrt(np.mean(np.log(model(N, B, K, tau) / av) ** 2))))
    return out
