"""The cases of the inertial seed (vc_seed_imu*), shared by tests/test_seed_imu_cpu.py (the host build of vc_seed_imu.hpp,
tests/host_harness/seed_imu_harness.cpp) and tests/test_seed_imu_gpu.py (the kernels).  The reference is tests/seed_imu_ref.py, run once per
group in float64 and in longdouble and kept.

A case is a problem (see seed_imu_ref.py) with `lags` to sweep and / or `pick` = (range_s, step_s, fine) to run the whole seed with.
  edges     1 and 2 valid intervals (status 1), 3, 4 and 5; one lag; a lag at which every interval leaves the log; a lag at which exactly
            max(3, min_intervals) stay and one at which one fewer does; tau exactly on the first and on the last sample; a frame that is
            not ok in the middle; a gap above max_gap_s
  sizes     intervals one below, at and one above 64, 256, the sweep's chunk, and two chunks plus one; samples 2, 3, around the scan's
            block and twice that, and the first size whose block totals need a second tile
  sampling  sample times jittered by +-30 % of the interval; one dropout of 20 intervals; a log shorter than the frames on either side
  truth     the generator's visual-inertial problem (synth.generate, kb4, 20 Hz frames, 200 Hz IMU, PnP-like rotations at 0.1 degrees):
            200 frames at the offsets 0.003, 0.12 and -0.2 s and 60 frames at 0.12 s: the builder holds the REFERENCE to the truth
Without a reference: `known` (a constant rate has no excitation; a two-axis rate in closed form gives R_ck, bias and offset back) and
`bytes`.  What runs a case is a backend with sweep(p, lags) and run(p, range_s, step_s, fine) returning the dicts of
vicalib_amd.lib.seed_imu_sweep / seed_imu: HostSeedImu here, DeviceSeedImu for the library.

The bound (one number): 100 times the largest spread between the reference's float64 and longdouble routes over all groups, on J relative
to Sa / n, the angle of R R_ref^T, the bias relative to the signal, the gravity angles, and the picked offset relative to the coarse step."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np

import seed_imu_ref as ref
from vicalib_amd import synth

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
GROUPS = ("edges", "sizes", "sampling", "truth")
R_CK_120 = np.array([[0.0, 1.0, 0.0], [0.0, 0.0, 1.0], [1.0, 0.0, 0.0]])          # a 120 degree rotation about (1, 1, 1): the generator's RDF_ROBOTICS
BIAS = np.array([0.002, -0.001, 0.0015])
G_DIR = np.array([0.03, -0.02])
# limits on the reference's error against the truth, three times its own measured worst, rounded up (DESIGN 4.19 has both figures):
# offset in s, rotation in degrees, gyro bias in rad/s, gravity angles in rad
TRUTH_LIMITS = dict(offset=2.5e-3, angle=1.4, bias=3.2e-3, g_dir=0.018)
TRUTH_CASES = ((200, 0.003), (200, 0.12), (200, -0.2), (60, 0.12))
FAIL_CASE = (20, 0.12)                  # one second of motion: the documented failure, recorded, not asserted


# ---------------------------------------------------------------------------------------------- the host build
def harness():
    src = os.path.join(HERE, "host_harness", "seed_imu_harness.cpp")
    so = os.path.join(HERE, "host_harness", "libvc_seed_imu_harness.so")
    deps = [src] + [os.path.join(ROOT, "vicalib_amd", "csrc", f) for f in ("vc_seed_imu.hpp", "vc_rectify.hpp", "vc_undistort.hpp", "vc_math.hpp")]
    if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(d) for d in deps):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-o", so, src])
    return C.CDLL(so)


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


@functools.lru_cache(maxsize=None)
def constants():
    out = (C.c_int * 6)()
    harness().seed_imu_harness_constants(out)
    return dict(scan_block=out[0], chunk=out[1], max_n=out[2], search_steps=out[3], moments=out[4], max_lags=out[5])


def _arrays(p):
    return (np.ascontiguousarray(p["frame_t"], dtype=np.float64), np.ascontiguousarray(p["frame_q"], dtype=np.float64),
            np.ascontiguousarray(np.asarray(p["frame_ok"]) != 0, dtype=np.uint8), np.ascontiguousarray(p["imu_t"], dtype=np.float64),
            np.ascontiguousarray(p["gyro"], dtype=np.float64), np.ascontiguousarray(p["accel"], dtype=np.float64))


class HostSeedImu:
    """the backend of the host build: the header's arithmetic in plain loops"""

    @staticmethod
    def sweep(p, lags):
        ft, fq, ok, it, g, a = _arrays(p)
        lags = np.ascontiguousarray(lags, dtype=np.float64)
        n = len(lags)
        J = np.zeros(n); R = np.zeros((n, 3, 3)); bias = np.zeros((n, 3)); count = np.zeros(n, dtype=np.int32); mom = np.zeros((n, 18))
        rc = harness().seed_imu_harness_sweep(len(ft), _p(ft), _p(fq), _p(ok), len(it), _p(it), _p(g), _p(a), C.c_double(p["max_gap_s"]), int(p["min_intervals"]), n,
                                              _p(lags), _p(J), _p(R), _p(bias), _p(count), _p(mom))
        assert rc == 0, rc
        return dict(J=J, R=R, bias=bias, count=count, moments=mom)

    @staticmethod
    def run(p, range_s, step_s, fine):
        ft, fq, ok, it, g, a = _arrays(p)
        out = np.zeros(17); ints = np.zeros(4, dtype=np.int32); cl = np.zeros(8192); cJ = np.zeros(8192)
        rc = harness().seed_imu_harness_run(len(ft), _p(ft), _p(fq), _p(ok), len(it), _p(it), _p(g), _p(a), C.c_double(p["max_gap_s"]), int(p["min_intervals"]),
                                            C.c_double(range_s), C.c_double(step_s), int(fine), _p(out), _p(ints), len(cl), _p(cl), _p(cJ))
        assert rc == 0 and ints[3] <= len(cl), (rc, ints)
        r = dict(status=int(ints[0]), coarse_lags=cl[:ints[3]].copy(), coarse_J=cJ[:ints[3]].copy())
        if r["status"] == 0:
            r.update(time_offset=out[0], R_ck=out[1:10].reshape(3, 3).copy(), gyro_bias=out[10:13].copy(), g_dir=out[13:15].copy(), rms=out[15], signal=out[16],
                     count=int(ints[1]))
        return r


class DeviceSeedImu:
    """the backend of the library: the kernels"""

    @staticmethod
    def _args(p):
        return p["frame_t"], p["frame_q"], p["frame_ok"], p["imu_t"], p["gyro"], p["accel"]

    @classmethod
    def sweep(cls, p, lags):
        import vicalib_amd.lib as lib
        return lib.seed_imu_sweep(*cls._args(p), lags, max_gap_s=p["max_gap_s"], min_intervals=p["min_intervals"])

    @classmethod
    def run(cls, p, range_s, step_s, fine):
        import vicalib_amd.lib as lib
        return lib.seed_imu(*cls._args(p), range_s=range_s, step_s=step_s, fine=fine, max_gap_s=p["max_gap_s"], min_intervals=p["min_intervals"])


# ---------------------------------------------------------------------------------------------- the problems
def _qmul(a, b):
    ax, ay, az, aw = a[..., 0], a[..., 1], a[..., 2], a[..., 3]
    bx, by, bz, bw = b[..., 0], b[..., 1], b[..., 2], b[..., 3]
    return np.stack([aw * bx + ax * bw + ay * bz - az * by, aw * by + ay * bw + az * bx - ax * bz, aw * bz + az * bw + ax * by - ay * bx,
                     aw * bw - ax * bx - ay * by - az * bz], axis=-1)


def _qexp(w):
    th = np.linalg.norm(w, axis=-1, keepdims=True)
    with np.errstate(divide="ignore", invalid="ignore"):
        k = np.where(th > 1e-12, np.sin(0.5 * th) / th, 0.5)
    return np.concatenate([k * w, np.cos(0.5 * th)], axis=-1)


A1, W1, P1, A2, W2, P2 = 0.6, 2 * np.pi / 3.1, 0.3, 0.5, 2 * np.pi / 4.7, 1.1


def motion(t):
    """R_wc(t) = Rz(alpha) Ry(beta) with two sinusoids, in closed form -> q_wc [n, 4], w_c [n, 3] (the camera-frame rate)"""
    t = np.asarray(t, dtype=np.float64)
    al, be = A1 * np.sin(W1 * t + P1), A2 * np.sin(W2 * t + P2)
    dal, dbe = A1 * W1 * np.cos(W1 * t + P1), A2 * W2 * np.cos(W2 * t + P2)
    z = np.zeros_like(t)
    q = _qmul(np.stack([z, z, np.sin(0.5 * al), np.cos(0.5 * al)], axis=-1), np.stack([z, np.sin(0.5 * be), z, np.cos(0.5 * be)], axis=-1))
    return q, np.stack([-dal * np.sin(be), dbe, dal * np.cos(be)], axis=-1)


def problem(frame_t, imu_t, offset=0.0, R_ck=R_CK_120, bias=BIAS, g_dir=G_DIR, sigma_r=np.deg2rad(0.1), seed=1, max_gap_s=0.5, min_intervals=10, ok=None):
    """frames and a log of the closed-form motion: gyro = R_ck^T w_c(t + offset) - bias, accel = the reaction to gravity alone"""
    frame_t = np.asarray(frame_t, dtype=np.float64); imu_t = np.asarray(imu_t, dtype=np.float64)
    q, _ = motion(frame_t)
    if sigma_r > 0.0:
        q = _qmul(q, _qexp(sigma_r * np.random.default_rng(seed).standard_normal((len(frame_t), 3))))
    qs, w = motion(imu_t + offset)
    gyro = w @ R_ck - bias                                                    # rows: R_ck^T w_c
    g_w = synth.gravity_vector(g_dir)
    accel = np.einsum("nji,j->ni", ref.quat_to_matrix(qs), g_w) @ R_ck        # R_ck^T R_wc^T g_w
    return dict(frame_t=frame_t, frame_q=q, frame_ok=np.ones(len(frame_t), dtype=np.uint8) if ok is None else np.asarray(ok, dtype=np.uint8), imu_t=imu_t,
                gyro=gyro, accel=accel, max_gap_s=max_gap_s, min_intervals=min_intervals,
                truth=dict(offset=offset, R_ck=R_ck, bias=bias, g_dir=np.asarray(g_dir, dtype=np.float64)))


def regular(n_int, frame_rate=20.0, imu_rate=200.0, pad=0.25, **kw):
    ft = 1.0 + np.arange(n_int + 1) / frame_rate
    n_s = int(np.ceil((ft[-1] - ft[0] + 2 * pad) * imu_rate)) + 1
    it = (ft[0] - pad) + np.arange(n_s) / imu_rate
    return problem(ft, it, **kw)


def with_samples(n_s, n_frames=6, **kw):
    """a log of exactly n_s samples around n_frames frames at 20 Hz, a quarter of a frame period of room on either side"""
    ft = 1.0 + np.arange(n_frames) / 20.0
    it = np.linspace(ft[0] - 0.0125, ft[-1] + 0.0125, n_s)
    return problem(ft, it, **kw)


def synth_problem(n_frames, offset, sigma_deg=0.1):
    prob = synth.generate(synth.Config(models=("kb4",), n_frames=n_frames, imu=True, imu_truth=dict(time_offset=offset), pose_sigma_r=np.deg2rad(sigma_deg)))
    return dict(frame_t=prob.frame_time, frame_q=prob.frame_T_wk_init[:, :4].copy(), frame_ok=np.ones(n_frames, dtype=np.uint8), imu_t=prob.imu_t, gyro=prob.imu_gyro,
                accel=prob.imu_accel, max_gap_s=0.5, min_intervals=10,
                truth=dict(offset=offset, R_ck=synth.quat_to_matrix(prob.cam_T_ck_gt[0, :4]), bias=prob.imu_gt["bg"], g_dir=prob.imu_gt["g_dir"]))


FEW_LAGS = np.array([-0.1, -0.013, 0.0, 0.0021, 0.02, 0.1])
PICK = (0.2, 0.0, 4)


def sizes_lists():
    c = constants()
    ch, B = c["chunk"], c["scan_block"]
    return [63, 64, 65, 255, 256, 257, ch - 1, ch, ch + 1, 2 * ch + 1], [2, 3, B - 1, B, B + 1, 2 * B - 1, 2 * B, 2 * B + 1, B * B + 1]


@functools.lru_cache(maxsize=None)
def group(name):
    if name == "edges":
        cases = []
        for v in (1, 2, 3, 4, 5):
            cases.append(dict(name="%d intervals" % v, p=regular(v, min_intervals=1, seed=10 + v), lags=np.array([0.0]), pick=(0.1, 0.0, 2)))
        # 11 intervals, the log from 0.9 to 1.7: at the lag 0.39 the intervals 6 .. 10 stay, at 0.44 four of them, at 1000 none
        p = problem(1.0 + 0.05 * np.arange(12), 0.9 + 0.005 * np.arange(161), min_intervals=5, seed=21)
        cases.append(dict(name="leaving the log", p=p, lags=np.array([0.39, 0.44, 1000.0, -1000.0, 0.0]), expect_count=[5, 4, 0, 0, 11]))
        # dyadic times: tau falls exactly on the first sample at the lag 0.5 and exactly on the last one at -0.25; one sample further loses an interval
        ft = 1.0 + np.arange(17) / 16.0
        it = 0.5 + np.arange(129) / 64.0                                         # 0.5 .. 2.5; the frames 1 .. 2
        p = problem(ft, it, min_intervals=3, seed=22)
        cases.append(dict(name="tau on a sample", p=p, lags=np.array([0.5, 0.5 + 1.0 / 64.0, -0.5, -0.5 - 1.0 / 64.0]), expect_count=[16, 15, 16, 15]))
        ok = np.ones(41, dtype=np.uint8); ok[20] = 0
        cases.append(dict(name="a frame not ok", p=regular(40, ok=ok, seed=23), lags=FEW_LAGS, pick=PICK, expect_count0=38))
        ft = np.delete(1.0 + np.arange(45) / 20.0, [20, 21, 22])                 # a gap of 0.2 s
        it = 0.75 + np.arange(541) / 200.0
        cases.append(dict(name="a gap", p=problem(ft, it, max_gap_s=0.12, seed=24), lags=FEW_LAGS, pick=PICK, expect_count0=40))
        return cases
    if name == "sizes":
        n_ints, n_samples = sizes_lists()
        cases = [dict(name="%d intervals" % n, p=regular(n, seed=100 + n), lags=FEW_LAGS, pick=PICK if n in (65, n_ints[-3]) else None) for n in n_ints]
        for n in n_samples:
            frames = 6 if n < 60000 else 1201
            p = with_samples(n, frames, min_intervals=3, seed=200 + n % 97)
            cases.append(dict(name="%d samples" % n, p=p, lags=np.array([-0.01, 0.0, 0.004, 0.0125, 0.02]), rotation=n > 2))
        return cases
    if name == "sampling":
        r = np.random.default_rng(5)
        ft = 1.0 + np.arange(121) / 20.0
        it = 0.75 + (np.arange(1301) + 0.3 * (2.0 * r.random(1301) - 1.0)) / 200.0
        cases = [dict(name="jitter", p=problem(ft, it, offset=0.02, seed=31), lags=FEW_LAGS, pick=PICK)]
        it = np.delete(0.75 + np.arange(1301) / 200.0, np.arange(600, 619))       # 19 samples out: one interval of 20
        cases.append(dict(name="dropout", p=problem(ft, it, offset=-0.03, seed=32), lags=FEW_LAGS, pick=PICK))
        it = 2.0 + np.arange(601) / 200.0                                         # 2 .. 5 of the frames' 1 .. 7
        cases.append(dict(name="short log", p=problem(ft, it, offset=0.01, seed=33), lags=FEW_LAGS, pick=PICK))
        return cases
    if name == "truth":
        return [dict(name="%d frames at %g s" % (n, off), p=synth_problem(n, off), lags=np.array([off - 0.005, off, off + 0.005]), pick=(0.5, 0.0, 8))
                for n, off in TRUTH_CASES]
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def reference(name):
    """per case: dict(sweep=(longdouble, float64) or None, pick=(longdouble, float64) or None)"""
    out = []
    for case in group(name):
        sw = tuple(ref.sweep(case["p"], case["lags"], dt) for dt in (np.longdouble, np.float64)) if case.get("lags") is not None else None
        pk = tuple(ref.seed(case["p"], *case["pick"], dtype=dt) for dt in (np.longdouble, np.float64)) if case.get("pick") else None
        out.append(dict(sweep=sw, pick=pk))
    return out


# ---------------------------------------------------------------------------------------------- the measures
def sweep_errors(got, want, rotation=True):
    """the largest error of J relative to Sa / n, of the angle of R R_ref^T and of the bias relative to the signal, over the lags with a fit;
    counts and the lags without a fit must agree exactly.  rotation = False: J alone (a log of two samples is one straight line per channel,
    the centred gyro rates span one direction, and the rotation about it is not determined: the cost is, the rotation and the bias are not)"""
    assert np.array_equal(np.asarray(got["count"]), np.asarray(want["count"])), (got["count"], want["count"])
    fin = np.isfinite(want["J"])
    assert np.array_equal(np.isfinite(got["J"]), fin) and np.all(np.asarray(got["J"])[~fin] == np.inf), (got["J"], want["J"])
    e = dict(J=0.0, angle=0.0, bias=0.0)
    for j in np.nonzero(fin)[0]:
        e["J"] = max(e["J"], abs(got["J"][j] - want["J"][j]) / want["Sa_n"][j])
        if not rotation:
            continue
        e["angle"] = max(e["angle"], ref.angle_between(got["R"][j], want["R"][j]))
        e["bias"] = max(e["bias"], float(np.max(np.abs(got["bias"][j] - want["bias"][j]))) / want["signal"][j])
    return e


def pick_errors(got, want):
    assert got["status"] == want["status"], (got["status"], want["status"])
    assert ref.argmin_finite(got["coarse_J"]) == want["coarse_index"] and len(got["coarse_J"]) == len(want["coarse_J"])
    np.testing.assert_allclose(got["coarse_lags"], want["coarse_lags"], rtol=0, atol=1e-15)
    if want["status"] != 0:
        return dict(offset=0.0, angle=0.0, bias=0.0, g_dir=0.0)
    assert got["count"] == want["count"], (got["count"], want["count"])
    return dict(offset=abs(got["time_offset"] - want["time_offset"]) / want["step"], angle=ref.angle_between(got["R_ck"], want["R_ck"]),
                bias=float(np.max(np.abs(got["gyro_bias"] - want["gyro_bias"]))) / want["signal"], g_dir=float(np.max(np.abs(got["g_dir"] - want["g_dir"]))),
                rms=abs(got["rms"] ** 2 - want["rms"] ** 2) / want["signal"] ** 2, signal=abs(got["signal"] - want["signal"]) / want["signal"])


def truth_errors(r, truth):
    return dict(offset=abs(r["time_offset"] - truth["offset"]), angle=np.rad2deg(ref.angle_between(r["R_ck"], truth["R_ck"])),
                bias=float(np.max(np.abs(r["gyro_bias"] - truth["bias"]))), g_dir=float(np.max(np.abs(r["g_dir"] - truth["g_dir"]))))


@functools.lru_cache(maxsize=None)
def bound():
    """-> (bound, spreads per group, the reference's worst error against the truth).  Asserts what the groups claim about themselves."""
    c = constants()
    n_ints, n_samples = sizes_lists()
    assert c["chunk"] == 1024 and c["scan_block"] == 256 and c["moments"] == 18 and c["max_n"] == 1 << 24 and c["search_steps"] == 25
    assert {63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 2049} == set(n_ints) and {2, 3, 255, 256, 257, 511, 512, 513, 65537} == set(n_samples)
    for case in group("sizes"):
        p = case["p"]
        assert case["name"] in ("%d intervals" % (len(p["frame_t"]) - 1), "%d samples" % len(p["imu_t"]))
    spreads = {}
    for name in GROUPS:
        worst = 0.0
        for case, r in zip(group(name), reference(name)):
            if r["sweep"]:
                ld, f64 = r["sweep"]
                worst = max(worst, *sweep_errors(f64, ld, case.get("rotation", True)).values())
                if "expect_count" in case:
                    assert ld["count"].tolist() == case["expect_count"], (case["name"], ld["count"])
                if "expect_count0" in case:
                    assert ld["count"][2] == case["expect_count0"], (case["name"], ld["count"])
            if r["pick"]:
                ld, f64 = r["pick"]
                worst = max(worst, *pick_errors(dict(f64), ld).values())
                J = ld["coarse_J"]; jc = ld["coarse_index"]
                if jc >= 0:                               # the argmin is well defined: no two costs within three steps of it closer than 1e-6 relative
                    near = J[max(0, jc - 3):jc + 4]; near = np.sort(near[np.isfinite(near)])
                    assert np.all(np.diff(near) > 1e-6 * near[1:]), (name, case["name"], near)
        spreads[name] = worst
    edges = {case["name"]: r for case, r in zip(group("edges"), reference("edges"))}
    assert [edges["%d intervals" % v]["pick"][0]["status"] for v in (1, 2)] == [1, 1]
    assert [int(edges["%d intervals" % v]["sweep"][0]["count"][0]) for v in (1, 2, 3, 4, 5)] == [1, 2, 3, 4, 5]
    assert np.isfinite(edges["leaving the log"]["sweep"][0]["J"]).tolist() == [True, False, False, False, True]
    for name in ("sizes", "sampling", "truth"):
        assert all(r["pick"][0]["status"] == 0 for r in reference(name) if r["pick"]), name
    # the reference against the truth
    worst = dict(offset=0.0, angle=0.0, bias=0.0, g_dir=0.0)
    for case, r in zip(group("truth"), reference("truth")):
        e = truth_errors(r["pick"][0], case["p"]["truth"])
        for k in worst:
            worst[k] = max(worst[k], e[k])
            assert e[k] <= TRUTH_LIMITS[k], (case["name"], k, e[k])
    b = 100.0 * max(spreads.values())
    assert 0.0 < b <= 1e-6, (b, spreads)
    return b, spreads, worst


def check(name, backend, label=""):
    """a backend on a group against the longdouble reference; prints the worst value over the bound"""
    b = bound()[0]
    worst = 0.0
    for case, r in zip(group(name), reference(name)):
        if r["sweep"]:
            e = sweep_errors(backend.sweep(case["p"], case["lags"]), r["sweep"][0], case.get("rotation", True))
            worst = max(worst, *e.values())
            assert max(e.values()) <= b, (name, case["name"], e, b)
        if r["pick"]:
            e = pick_errors(backend.run(case["p"], *case["pick"]), r["pick"][0])
            worst = max(worst, *e.values())
            assert max(e.values()) <= b, (name, case["name"], e, b)
    print("seed_imu %s%s: worst error %.3g of the bound %.3g" % (name, label, worst / b, b))
    return worst / b


# ---------------------------------------------------------------------------------------------- known answers
@functools.lru_cache(maxsize=None)
def known_cases():
    """-> (constant-rate problem, its rate; the noise-free two-axis problem, its pick, the reference's error against its truth)"""
    rate = np.array([0.3, -0.2, 0.5])
    ft = 1.0 + np.arange(41) / 20.0
    it = 0.75 + np.arange(501) / 200.0
    q = _qexp((ft - ft[0])[:, None] * rate[None, :])
    const = dict(frame_t=ft, frame_q=q, frame_ok=np.ones(41, dtype=np.uint8), imu_t=it, gyro=np.tile(rate @ R_CK_120, (501, 1)), accel=np.tile([0.0, 9.8, 0.0], (501, 1)),
                 max_gap_s=0.5, min_intervals=10)
    r = ref.sweep(const, [0.0])
    assert r["count"][0] == 40 and r["signal"][0] < 1e-9 * np.linalg.norm(rate), r["signal"]
    two = regular(400, offset=0.0375, sigma_r=0.0, pad=0.3)
    pick = (0.25, 0.0, 8)
    rr = ref.seed(two, *pick)
    assert rr["status"] == 0
    err = truth_errors(rr, two["truth"])
    assert err["offset"] < 1e-3 and err["angle"] < 0.1 and err["bias"] < 1e-3 and err["g_dir"] < 1e-3, err      # (second order in |w| dt, not rounding)
    return const, rate, two, pick, err


def signal_of(moments):
    m = np.asarray(moments, dtype=np.float64)
    sa = m[7] - (m[1] * m[1] + m[2] * m[2] + m[3] * m[3]) / m[0]
    return float(np.sqrt(max(sa, 0.0) / m[0]))


def check_known(backend, label=""):
    const, rate, two, pick, err = known_cases()
    got = backend.sweep(const, [0.0])
    s = signal_of(got["moments"][0])
    print("seed_imu known%s: constant rate: signal %.3g of the rate" % (label, s / np.linalg.norm(rate)))
    assert got["count"][0] == 40 and s < 1e-9 * np.linalg.norm(rate), s
    r = backend.run(two, *pick)
    assert r["status"] == 0
    e = truth_errors(r, two["truth"])
    print("seed_imu known%s: two axes: errors %s; the reference's %s" % (label, e, err))
    for k in e:
        assert e[k] <= 10.0 * err[k], (k, e[k], err[k])


# ---------------------------------------------------------------------------------------------- bytes
def check_bytes(backend):
    p = group("sizes")[8]["p"]                       # one interval more than a chunk
    lag = np.array([0.0021])
    alone = backend.sweep(p, lag)
    again = backend.sweep(p, lag)
    for k in ("J", "R", "bias", "count", "moments"):
        assert alone[k].tobytes() == again[k].tobytes(), k
    many = np.concatenate([np.linspace(-0.2, 0.2, 100), lag, np.linspace(-0.15, 0.25, 100)])
    among = backend.sweep(p, many)
    for k in ("J", "R", "bias", "count", "moments"):
        assert alone[k][0].tobytes() == among[k][100].tobytes(), k
    a, b = backend.run(p, *PICK), backend.run(p, *PICK)
    assert a["status"] == 0 and all(np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes() for k in a)
    # the three gyro channels permuted cyclically: b'_j = b_perm[j], so R' = R[:, perm]: the same J bits, the columns of R and the bias permuted
    base = backend.sweep(p, FEW_LAGS)
    for perm in ([1, 2, 0], [2, 0, 1]):
        q = dict(p, gyro=np.ascontiguousarray(p["gyro"][:, perm]))
        got = backend.sweep(q, FEW_LAGS)
        assert got["J"].tobytes() == base["J"].tobytes(), perm
        assert np.ascontiguousarray(base["R"][:, :, perm]).tobytes() == got["R"].tobytes(), perm
        assert np.ascontiguousarray(base["bias"][:, perm]).tobytes() == got["bias"].tobytes(), perm
