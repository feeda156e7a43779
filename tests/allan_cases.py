"""The cases of the IMU noise characterisation (vc_allan*), shared by tests/test_allan_cpu.py (the host build of vc_allan.hpp,
tests/host_harness/allan_harness.cpp) and tests/test_allan_gpu.py (the kernels).  The reference is tests/allan_ref.py, run once per group and kept.

A group is a list of logs (gyro [n, 3], accel [n, 3], time [n]) with the factors to run and, optionally, a sub-range.
  edges     n = 2, 3, 4, 5 with every legal factor; a range of 20 samples inside a log of 40 with the factors 1 and 10: at 10 one term
  sizes     n one below, at and one above the scan's block size, twice that, the sweep's chunk length (in samples and in terms at m = 1)
            and the first size whose block totals need a second tile; factors 4 per decade up to n / 2
  noise     seeds 1, 2, 3: n = 65 536 at tau0 = 0.005, gx white noise of sigma 2e-3 alone, ax the same noise with a random walk of
            K = 3e-4; 10 factors per decade up to 1/9
  range     one log of 3000 samples, whole, on samples [517, 517 + 1301), and whole again
Without a reference: `known` (a constant, a ramp, +1 -1 +1 ...), `channels` (bytes), `static` (integers).
What runs a log is a "session": open(gyro, accel, time) -> an object with run(m) -> (avar [6, n_m], terms), set_range(first, count),
static(window, gyro_thr, accel_thr) -> (status, first, count, n_quiet), get() and close(): HostAllan here, vicalib_amd.lib.AllanAnalyzer
on the device.  The bound on adev is relative, per point: 100 times the largest spread between the reference's float64 and longdouble
routes over all groups."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np

import allan_ref as ref

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
GROUPS = ("edges", "sizes", "noise", "range")
TAU0 = 0.005
SIGMA, RW_K = 2e-3, 3e-4


# ---------------------------------------------------------------------------------------------- the host build
def harness():
    src = os.path.join(HERE, "host_harness", "allan_harness.cpp")
    so = os.path.join(HERE, "host_harness", "libvc_allan_harness.so")
    deps = [src] + [os.path.join(ROOT, "vicalib_amd", "csrc", f) for f in ("vc_allan.hpp", "vc_imu_weights.hpp", "vc_imu.hpp", "vc_math.hpp")]
    if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(d) for d in deps):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-o", so, src])
    L = C.CDLL(so)
    return L


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


@functools.lru_cache(maxsize=None)
def constants():
    out = (C.c_int * 4)()
    harness().allan_harness_constants(out)
    return dict(scan_block=out[0], chunk=out[1], max_n=out[2], second_tile=out[3])


class HostAllan:
    """the session of the host build: the header's arithmetic in plain loops"""

    def __init__(self, gyro, accel, time):
        self.L = harness()
        g = np.ascontiguousarray(gyro, dtype=np.float64); a = np.ascontiguousarray(accel, dtype=np.float64)
        self.n = len(g)
        self.means = np.zeros(6); self.S = np.zeros((6, self.n + 1))
        self.L.allan_harness_prefix(self.n, _p(g), _p(a), _p(self.means), _p(self.S))
        self.first, self.count = 0, self.n
        self.info = ref.log_info(time)

    def close(self):
        pass

    def get(self):
        tau0, lo, hi, irr = self.info
        return dict(n=self.n, tau0=tau0, dt_min=lo, dt_max=hi, means=self.means, irregular=irr, range=(self.first, self.count))

    def set_range(self, first, count):
        assert first >= 0 and count >= 2 and first + count <= self.n
        self.first, self.count = first, count

    def run(self, m):
        m = np.ascontiguousarray(m, dtype=np.int32)
        avar = np.zeros((6, len(m))); terms = np.zeros(len(m), dtype=np.int32)
        assert self.L.allan_harness_avar(self.n, _p(self.S), self.first, self.count, len(m), _p(m), _p(avar), _p(terms)) == 0
        return avar, terms

    def static(self, window, gyro_thr=0.0, accel_thr=0.0):
        rng = (C.c_int * 2)(self.first, self.count); nq = C.c_int(0)
        st = self.L.allan_harness_static(self.n, _p(self.S), int(window), C.c_double(gyro_thr), C.c_double(accel_thr), rng, C.byref(nq))
        if st == 0:
            self.first, self.count = rng[0], rng[1]
        return st, rng[0], rng[1], nq.value


def host_fit(tau, avar, e):
    tau, avar, e = (np.ascontiguousarray(a, dtype=np.float64) for a in (tau, avar, e))
    out = np.zeros(5); mask = C.c_int(0)
    st = harness().allan_harness_fit(len(tau), _p(tau), _p(avar), _p(e), _p(out), C.byref(mask))
    return dict(N=out[0], B=out[1], K=out[2], rms_log=out[3], n_points=int(out[4]), mask=mask.value, status=st)


def host_factors(n_used, per_decade, max_fraction):
    m = np.zeros(4096, dtype=np.int32); e = np.zeros(4096)
    k = harness().allan_harness_factors(int(n_used), int(per_decade), C.c_double(max_fraction), len(m), _p(m), _p(e))
    return m[:k], e[:k]


# ---------------------------------------------------------------------------------------------- the logs
def _time(n, tau0=TAU0):
    return 100.0 + tau0 * np.arange(n)


def _noise_log(n, seed, scale=1.0):
    """six channels of white noise, different sigmas, a small offset and gravity on az"""
    r = np.random.default_rng(seed)
    g = scale * SIGMA * r.standard_normal((n, 3)) * np.array([1.0, 0.7, 1.6]) + np.array([1e-3, -2e-3, 5e-4])
    a = scale * 10 * SIGMA * r.standard_normal((n, 3)) * np.array([0.9, 1.3, 1.0]) + np.array([0.02, -0.01, 9.81])
    return dict(gyro=g, accel=a, time=_time(n))


def sizes_list():
    c = constants()
    B, ch, t2 = c["scan_block"], c["chunk"], c["second_tile"]
    ns = [B - 1, B, B + 1, 2 * B - 1, 2 * B, 2 * B + 1, ch - 1, ch, ch + 1, ch + 2]
    if t2 <= 1 << 18:
        ns += [t2 - 1, t2, t2 + 1]
    return ns


def _factors_to_half(n, per_decade=4):
    m = ref.factors(n, per_decade, 0.5).tolist()
    if m[-1] != n // 2:
        m.append(n // 2)
    return np.array(m, dtype=np.int32)


def noise_truth():
    return dict(N=SIGMA * np.sqrt(TAU0), K=RW_K)


@functools.lru_cache(maxsize=None)
def group(name):
    """-> list of dict(gyro, accel, time, steps): steps is a list of (range or None, factors) run one after the other on one session"""
    if name == "edges":
        logs = []
        for n in (2, 3, 4, 5):
            logs.append(dict(_noise_log(n, 40 + n), steps=[(None, np.arange(1, n // 2 + 1, dtype=np.int32))]))
        logs.append(dict(_noise_log(40, 49), steps=[((3, 20), np.array([1, 10], dtype=np.int32))]))
        return logs
    if name == "sizes":
        return [dict(_noise_log(n, 1000 + n), steps=[(None, _factors_to_half(n))]) for n in sizes_list()]
    if name == "noise":
        n = 65536
        m = ref.factors(n, 10, 1.0 / 9.0)
        logs = []
        for seed in (1, 2, 3):
            r = np.random.default_rng(seed)
            white = SIGMA * r.standard_normal(n)
            walk = RW_K * np.sqrt(TAU0) * np.cumsum(r.standard_normal(n))
            log = _noise_log(n, 100 + seed)
            log["gyro"][:, 0] = white
            log["accel"][:, 0] = white + walk
            logs.append(dict(log, steps=[(None, m)]))
        return logs
    if name == "range":
        n = 3000
        return [dict(_noise_log(n, 7), steps=[(None, ref.factors(n, 10, 1.0 / 9.0)), ((517, 1301), ref.factors(1301, 10, 0.5)), (None, ref.factors(n, 10, 1.0 / 9.0))])]
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def reference(name):
    """-> (per log, per step: avar [6, n_m] of the longdouble route, the float64 route)"""
    out = []
    for log in group(name):
        steps = []
        for rng, m in log["steps"]:
            first, count = rng if rng else (0, None)
            steps.append((ref.avar6(log["gyro"], log["accel"], m, first, count, np.longdouble), ref.avar6(log["gyro"], log["accel"], m, first, count, np.float64)))
        out.append(steps)
    return out


def _rel(a, b):
    return float(np.max(np.abs(np.sqrt(a) - np.sqrt(b)) / np.sqrt(b)))


@functools.lru_cache(maxsize=None)
def bound():
    """-> (bound, spreads per group).  Asserts what the groups claim about themselves and about the reference."""
    c = constants()
    ns = sizes_list()
    for edge in (c["scan_block"], 2 * c["scan_block"], c["chunk"]):
        assert {edge - 1, edge, edge + 1} <= set(ns), edge
    assert {c["chunk"], c["chunk"] + 1, c["chunk"] + 2} <= set(ns)                     # terms at m = 1: chunk - 1, chunk, chunk + 1
    assert c["second_tile"] == c["scan_block"] ** 2 + 1 and (c["second_tile"] > 1 << 18 or {c["second_tile"] - 1, c["second_tile"], c["second_tile"] + 1} <= set(ns))
    edges = group("edges")
    assert [len(l["time"]) for l in edges[:4]] == [2, 3, 4, 5] and all(len(l["steps"][0][1]) == len(l["time"]) // 2 for l in edges[:4])
    (rng, m), = edges[4]["steps"]
    assert ref.terms(rng[1], int(m[-1])) == 1
    spreads = {}
    for name in GROUPS:
        spreads[name] = max(_rel(f64, ld) for steps in reference(name) for ld, f64 in steps)
    # the noise group: the reference against the truth
    truth = noise_truth()
    worst = dict(curve=0.0, N=0.0, K=0.0)
    for log, steps in zip(group("noise"), reference("noise")):
        m = log["steps"][0][1]
        tau, e = TAU0 * m, ref.rel_err(len(log["time"]), m)
        adev = np.sqrt(steps[0][0])
        worst["curve"] = max(worst["curve"], float(np.max(np.abs(adev[0] / (truth["N"] / np.sqrt(tau)) - 1.0) / e)))
        f_white, f_walk = ref.fit(tau, steps[0][0][0], e), ref.fit(tau, steps[0][0][3], e)
        assert f_white["status"] == 0 and f_walk["status"] == 0 and (f_walk["mask"] & 5) == 5
        worst["N"] = max(worst["N"], abs(f_white["N"] / truth["N"] - 1.0), abs(f_walk["N"] / truth["N"] - 1.0))
        worst["K"] = max(worst["K"], abs(f_walk["K"] / truth["K"] - 1.0))
    assert worst["curve"] <= 4.0 and worst["N"] <= 0.02 and worst["K"] <= 0.15, worst
    b = 100.0 * max(spreads.values())
    assert 0.0 < b <= 1e-6, (b, spreads)
    return b, spreads, worst


def run_group(name, open_session):
    """every step of every log of the group -> per log, per step: (avar, terms)"""
    out = []
    for log in group(name):
        s = open_session(log["gyro"], log["accel"], log["time"])
        steps = []
        for rng, m in log["steps"]:
            s.set_range(*(rng if rng else (0, len(log["time"]))))
            steps.append(s.run(m))
        s.close()
        out.append(steps)
    return out


def check(name, got, label=""):
    """adev of every point within the bound of the reference, relative; the term counts exactly.  Returns the worst value over the bound."""
    b = bound()[0]
    worst = 0.0
    for log, want_steps, got_steps in zip(group(name), reference(name), got):
        for (rng, m), (ld, _), (avar, terms) in zip(log["steps"], want_steps, got_steps):
            count = rng[1] if rng else len(log["time"])
            assert terms.tolist() == [ref.terms(count, int(x)) for x in m], (name, label)
            assert avar.shape == ld.shape and np.all(np.isfinite(avar)) and np.all(avar >= 0.0)
            worst = max(worst, _rel(avar, ld) / b)
    print("allan %s%s: worst adev error / bound %.3e (bound %.3e)" % (name, label, worst, b))
    assert worst <= 1.0, (name, label, worst)
    return worst


# ---------------------------------------------------------------------------------------------- known answers
def check_known(open_session, label=""):
    n = 4097
    t = _time(n)
    # a constant: adev <= 1e-12 |c|
    c = np.array([0.3, -1.7, 9.81, 1e-3, 250.0, -1e-6])
    m = ref.factors(n, 10, 0.5)
    s = open_session(np.tile(c[:3], (n, 1)), np.tile(c[3:], (n, 1)), t)
    avar, _ = s.run(m); s.close()
    worst_c = float(np.max(np.sqrt(avar) / np.abs(c)[:, None]))
    assert worst_c <= 1e-12, (label, worst_c)
    # a ramp y = a t: adev = a tau / sqrt 2 to 1e-10 relative
    a = np.array([0.37, -1.3, 2.5e-3, 7.0, -0.011, 1.0])
    y = a[None, :] * (t - t[0])[:, None]
    s = open_session(y[:, :3], y[:, 3:], t)
    avar, _ = s.run(m); s.close()
    want = np.abs(a)[:, None] * (TAU0 * m)[None, :] / np.sqrt(2.0)
    worst_r = float(np.max(np.abs(np.sqrt(avar) / want - 1.0)))
    assert worst_r <= 1e-10, (label, worst_r)
    # +1, -1, +1, ... at tau0 = 1 (an even count: the mean is exactly 0): avar = 2 / m^2 for odd m, exactly 2 at m = 1, 0 for even m
    n = 1024
    alt = np.where(np.arange(n) % 2 == 0, 1.0, -1.0)
    y = np.tile(alt[:, None], (1, 3))
    m = np.arange(1, 41, dtype=np.int32)
    s = open_session(y, -y, np.arange(n, dtype=np.float64))
    avar, _ = s.run(m); s.close()
    assert np.all(avar[:, 0] == 2.0), (label, avar[:, 0])
    odd = m % 2 == 1
    worst_a = float(np.max(np.abs(avar[:, odd] * (m[odd].astype(np.float64) ** 2) / 2.0 - 1.0)))
    worst_e = float(np.max(avar[:, ~odd]))
    assert worst_a <= 1e-14 and worst_e == 0.0, (label, worst_a, worst_e)
    print("allan known%s: constant %.2e, ramp %.2e, alternating odd %.2e even %.2e" % (label, worst_c, worst_r, worst_a, worst_e))


# ---------------------------------------------------------------------------------------------- a channel alone, and again
def check_channels(open_session):
    n = constants()["chunk"] + 700
    log = _noise_log(n, 5)
    ch = ref.channels(log["gyro"], log["accel"])
    ch[1] += 1e-3 * np.cumsum(np.random.default_rng(6).standard_normal(n))      # six different signals: a walk, a ramp, a sine, a step
    ch[2] += 1e-5 * np.arange(n)
    ch[3] += 0.3 * np.sin(0.01 * np.arange(n))
    ch[4][n // 2:] += 0.5
    m = ref.factors(n, 10, 1.0 / 9.0)

    def run(c6):
        s = open_session(np.ascontiguousarray(c6[:3].T), np.ascontiguousarray(c6[3:].T), log["time"])
        first, _ = s.run(m)
        again, _ = s.run(m)
        means = s.get()["means"].copy()
        s.close()
        assert first.tobytes() == again.tobytes()
        return first, means
    full, means = run(ch)
    assert run(ch)[0].tobytes() == full.tobytes()                              # a second handle
    for c in range(6):
        alone = np.zeros_like(ch)
        alone[c] = ch[c]
        got, mu = run(alone)
        assert got[c].tobytes() == full[c].tobytes() and mu[c].tobytes() == means[c].tobytes(), c
        assert np.all(np.delete(got, c, axis=0) == 0.0)


# ---------------------------------------------------------------------------------------------- the static stretch
STATIC_W = 100
STATIC_THR = (5e-3, 5e-2)


@functools.lru_cache(maxsize=None)
def static_log():
    """rest, a burst of motion, a longer rest, a burst: samples [0, 1500) [1500, 1700) [1700, 5300) [5300, 5500) [5500, 6000)"""
    n = 6000
    log = _noise_log(n, 11)
    r = np.random.default_rng(12)
    for a, b in ((1500, 1700), (5300, 5500)):
        log["gyro"][a:b] += 0.5 * r.standard_normal((b - a, 3))
        log["accel"][a:b] += 3.0 * r.standard_normal((b - a, 3))
    q = ref.window_change(log["gyro"], log["accel"], STATIC_W)
    for k in (0, 1):                        # no statistic within 1e-6 relative of its threshold: rounding cannot move the answer
        assert np.min(np.abs(q[k] / STATIC_THR[k] - 1.0)) > 1e-6
    q_ld = ref.window_change(log["gyro"], log["accel"], STATIC_W, np.longdouble)
    assert np.max(np.abs(q / q_ld - 1.0)) < 1e-9
    return log


def check_static(open_session):
    log = static_log()
    n = len(log["time"])
    cases = [STATIC_THR, (STATIC_THR[0], 0.0), (0.0, STATIC_THR[1]), (0.0, 0.0), (-1.0, -1.0)]
    for g_thr, a_thr in cases:
        want = ref.static(log["gyro"], log["accel"], STATIC_W, g_thr, a_thr)
        s = open_session(log["gyro"], log["accel"], log["time"])
        got = s.static(STATIC_W, g_thr, a_thr)
        assert tuple(got) == tuple(want), (g_thr, a_thr, got, want)
        assert s.get()["range"] == (want[1], want[2])
        if g_thr > 0 and a_thr > 0:
            assert 1650 <= want[1] <= 1750 and 5250 <= want[1] + want[2] <= 5350, want      # the longer rest, less what the bursts reach into
        else:
            assert g_thr > 0 or a_thr > 0 or (want[1], want[2]) == (0, n)
        # the sweep over the range found is the reference's on that slice
        m = ref.factors(want[2], 5, 1.0 / 9.0)
        avar, _ = s.run(m)
        assert _rel(avar, ref.avar6(log["gyro"], log["accel"], m, want[1], want[2], np.longdouble)) <= bound()[0]
        s.close()
    # no quiet start: status 1, the range as it was
    s = open_session(log["gyro"], log["accel"], log["time"])
    s.set_range(10, 500)
    assert ref.static(log["gyro"], log["accel"], STATIC_W, 1e-9, 1e-9)[0] == 1
    st, first, count, nq = s.static(STATIC_W, 1e-9, 1e-9)
    assert (st, first, count, nq) == (1, 10, 500, 0) and s.get()["range"] == (10, 500)
    s.close()


# ---------------------------------------------------------------------------------------------- the fit
@functools.lru_cache(maxsize=None)
def fit_cases():
    """the reference's own curves of the noise group (white alone: gx; with a walk: ax) and three synthetic curves with a 2 % ripple:
    all three terms, B alone (the ripple brings a little N in) and three points of N alone"""
    out = []
    for log, steps in zip(group("noise"), reference("noise")):
        m = log["steps"][0][1]
        tau, e = TAU0 * m, ref.rel_err(len(log["time"]), m)
        out += [(tau, steps[0][0][0], e), (tau, steps[0][0][3], e)]
    m = ref.factors(1 << 20, 10, 1.0 / 9.0)
    tau, e = TAU0 * m, ref.rel_err(1 << 20, m)
    wiggle = 1.0 + 0.02 * np.sin(np.arange(len(m)))
    out.append((tau, ref.model(1e-4, 3e-5, 2e-5, tau) * wiggle, e))
    out.append((tau, ref.model(0.0, 3e-5, 0.0, tau) * wiggle, e))
    out.append((tau[:3], ref.model(1e-4, 0.0, 0.0, tau[:3]) * wiggle[:3], e[:3]))
    return out


@functools.lru_cache(maxsize=None)
def fit_bound():
    spread = 0.0
    refs = []
    for tau, av, e in fit_cases():
        a, b = ref.fit(tau, av, e, "normal"), ref.fit(tau, av, e, "lstsq")
        assert a["status"] == b["status"] == 0 and a["mask"] == b["mask"], (a, b)
        spread = max(spread, _fit_diff(a, b))
        refs.append(b)
    bnd = 100.0 * spread
    assert 0.0 < bnd <= 1e-6, bnd
    return bnd, refs


def _fit_diff(got, want):
    d = abs(got["rms_log"] - want["rms_log"])
    for k, bit in (("N", 1), ("B", 2), ("K", 4)):
        d = max(d, abs(got[k] / want[k] - 1.0) if want["mask"] & bit else abs(got[k]))
    return d


def check_fit(fit_fn, label=""):
    bnd, refs = fit_bound()
    worst = 0.0
    for (tau, av, e), want in zip(fit_cases(), refs):
        got = fit_fn(tau, av, e)
        assert got["status"] == 0 and got["mask"] == want["mask"] and got["n_points"] == len(tau), (got, want)
        worst = max(worst, _fit_diff(got, want) / bnd)
    print("allan fit%s: worst / bound %.3e (bound %.3e)" % (label, worst, bnd))
    assert worst <= 1.0, worst
    assert {r["mask"] for r in refs} >= {1, 3, 5, 7}                             # N alone, N + B, N + K, all three
    # refusals: fewer than three usable points; points that are not positive and finite are left out
    tau, av, e = fit_cases()[6]
    assert fit_fn(tau[:2], av[:2], e[:2])["status"] == 1
    bad = av.copy(); bad[3:] = 0.0; bad[0] = np.nan
    assert fit_fn(tau, bad, e)["status"] == 1
    holes = av.copy(); holes[5] = np.inf; holes[9] = -1.0
    keep = np.ones(len(tau), dtype=bool); keep[[5, 9]] = False
    a, b = fit_fn(tau, holes, e), fit_fn(tau[keep], av[keep], e[keep])
    assert a == b and a["n_points"] == len(tau) - 2
    return worst


if __name__ == "__main__":
    b, spreads, worst = bound()
    print("bound %.3e; spreads %s; reference against the truth %s" % (b, {k: "%.2e" % v for k, v in spreads.items()}, {k: "%.3g" % v for k, v in worst.items()}))
    for name in GROUPS:
        check(name, run_group(name, HostAllan), label=" (host build)")
    check_known(HostAllan, " (host build)")
    check_channels(HostAllan)
    check_static(HostAllan)
    check_fit(host_fit, " (host build)")
