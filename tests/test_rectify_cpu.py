"""Stereo rectification (vc_stereo_*, vc_match_tiles, vc_rectif*), the part that needs no GPU: the rotations and the common intrinsics (host
entry points of the library), the corner matcher, the command line's flags, the refusal to run without a device, and the check's arithmetic
(vc_rectify.hpp) compiled for the host and held to the same numpy reference that tests/test_rectify_gpu.py applies to the kernel."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

import rectify_cases as rc
import undistort_cases as uc
import vicalib_amd.lib as lib
from vicalib_amd import synth
from vicalib_amd.lib import Rectifier
from test_undistort_cpu import host_map, host_points

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
BIN = os.path.join(ROOT, "vicalib_amd", "vicalib")


def _have_gpu():
    try:
        import torch
        return torch.cuda.is_available()
    except Exception:
        return False


def _harness():
    src = os.path.join(HERE, "host_harness", "rectify_harness.cpp")
    so = os.path.join(HERE, "host_harness", "libvc_rectify_harness.so")
    deps = [src] + [os.path.join(ROOT, "vicalib_amd", "csrc", f) for f in ("vc_rectify.hpp", "vc_undistort.hpp", "vc_math.hpp")]
    if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(d) for d in deps):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-o", so, src])
    return C.CDLL(so)


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def host_rotations(Ta, Tb):
    Ra, Rb, b = np.zeros((3, 3)), np.zeros((3, 3)), C.c_double(0)
    st = _harness().vrh_rotations(_p(np.ascontiguousarray(Ta)), _p(np.ascontiguousarray(Tb)), _p(Ra), _p(Rb), C.byref(b))
    return st, Ra, Rb, b.value


def host_check(c, dl=rc.DST_LINEAR, with_target=True):
    """the host build of the whole check on a case, in the layout Rectifier.check returns"""
    Ra, Rb, b = Rectifier.rotations(c.T_ck[0], c.T_ck[1])
    n, nf = len(c.px_a), len(c.frame_off) - 1
    pairs = np.zeros((n, 6)); flags = np.zeros(n, dtype=np.uint8); stats = np.zeros((nf, 8))
    m = [synth.MODEL_IDS[x] for x in c.models]
    px_a, px_b, tg = np.ascontiguousarray(c.px_a), np.ascontiguousarray(c.px_b), np.ascontiguousarray(c.target)
    _harness().vrh_check(m[0], _p(c.K[0]), len(c.K[0]), _p(Ra), m[1], _p(c.K[1]), len(c.K[1]), _p(Rb), _p(dl), C.c_double(b), nf, _p(c.frame_off), _p(px_a), _p(px_b),
                         _p(tg) if with_target else None, _p(pairs), _p(flags), _p(stats))
    return dict(pairs=pairs, invalid=flags.astype(bool), count=stats[:, 0].astype(int), n_invalid=stats[:, 1].astype(int), sum_dv=stats[:, 2], sum_dv2=stats[:, 3],
                max_abs_dv=stats[:, 4], worst=stats[:, 5].astype(np.int64), mean_z=stats[:, 6], rigid_rms=stats[:, 7]), Ra


# ---------------------------------------------------------------------------------------------------------------- rotations
@pytest.mark.parametrize("name", ["fov-fov", "kb4-poly3", "hand", "hand-left"])
def test_rotations(name):
    Ta, Tb = rc.rigs()[name]
    Ra, Rb, b = Rectifier.rotations(Ta, Tb)
    rc.check_rotations(Ta, Tb, Ra, Rb, b)
    wa, wb, wbase = rc.numpy_rotations(Ta, Tb)
    assert np.abs(Ra - wa).max() <= 1e-12 and np.abs(Rb - wb).max() <= 1e-12 and abs(b - wbase) <= 1e-12
    # the header's arithmetic compiled for the host is what the library runs
    st, ha, hb, hbase = host_rotations(Ta, Tb)
    assert st == 0 and np.array_equal(ha, Ra) and np.array_equal(hb, Rb) and hbase == b
    assert (b < 0) == (name == "hand-left")
    # a and b exchanged: the baseline changes its sign, the two rectified frames stay
    Sa, Sb, sbase = Rectifier.rotations(Tb, Ta)
    assert abs(sbase + b) <= 1e-12 and np.abs(Sa - Rb).max() <= 1e-12 and np.abs(Sb - Ra).max() <= 1e-12


def test_rotations_refuse_vertical_and_coincident_rigs():
    L = lib.load()
    out = np.zeros(9); b = C.c_double(0)
    Ta, Tb = rc.vertical_rig()
    assert L.vc_stereo_rectify_rotations(_p(Ta), _p(Tb), _p(out), _p(out), C.byref(b)) == -7       # VC_ERR_UNSUPPORTED
    assert L.vc_stereo_rectify_rotations(_p(Ta), _p(Ta.copy()), _p(out), _p(out), C.byref(b)) == -6      # VC_ERR_NUMERIC
    near = rc.pose(np.eye(3), [5e-10, 0, 0])
    assert L.vc_stereo_rectify_rotations(_p(Ta), _p(near), _p(out), _p(out), C.byref(b)) == -6
    bad = Ta.copy(); bad[3] = 1.1
    assert L.vc_stereo_rectify_rotations(_p(bad), _p(Tb), _p(out), _p(out), C.byref(b)) == -2
    assert host_rotations(Ta, Tb)[0] == 2 and host_rotations(Ta, Ta)[0] == 1


def test_rectified_poses_differ_by_an_x_translation():
    """T_ck_rect = (R_ds R_ck, R_ds t_ck) as vc_rectifier_get forms it, from the rotations alone"""
    for Ta, Tb in rc.rigs().values():
        Ra, Rb, b = Rectifier.rotations(Ta, Tb)
        (Rak, tak), (Rbk, tbk) = rc.pose_Rt(Ta), rc.pose_Rt(Tb)
        assert np.abs(Ra @ Rak - Rb @ Rbk).max() <= 1e-12
        assert np.abs((Rb @ tbk - Ra @ tak) - [-b, 0, 0]).max() <= 1e-12


# ---------------------------------------------------------------------------------------------------------------- common intrinsics
FIT_RIGS = [("kb4", "poly3"), ("fov", "fov"), ("rational6", "poly2")]


@pytest.mark.parametrize("models", FIT_RIGS)
def test_stereo_fit_alpha0_every_destination_pixel_valid_on_both_sides(models):
    Ta, Tb = rc.generator_rig(models)
    Ra, Rb, _ = Rectifier.rotations(Ta, Tb)
    dst = (163, 121)
    cams = [(m, uc.gt(m), uc.FULL) for m in models]
    dl = Rectifier.fit_linear(cams[0], Ra, cams[1], Rb, dst, alpha=0.0)
    inside_by = []
    for (m, K, size), R in zip(cams, (Ra, Rb)):
        mp, valid = host_map(m, K, size, dl, dst, R)
        assert valid.all(), (m, (~valid).sum())
        edge = np.concatenate([mp[0], mp[-1], mp[:, 0], mp[:, -1]]).astype(np.float64)
        inside_by.append(np.minimum(np.minimum(edge[:, 0], size[0] - 1 - edge[:, 0]), np.minimum(edge[:, 1], size[1] - 1 - edge[:, 1])).min())
    # ... and not by much: on every side of the rectangle one of the two cameras is the limit; the loosest test that still sees a rectangle
    # drawn in too far is that some border pixel lies within a few source pixels of a source border
    assert min(inside_by) < 4.0, inside_by


@pytest.mark.parametrize("models", FIT_RIGS)
def test_stereo_fit_alpha1_keeps_every_source_pixel(models):
    Ta, Tb = rc.generator_rig(models)
    Ra, Rb, _ = Rectifier.rotations(Ta, Tb)
    dst = (163, 121)
    cams = [(m, uc.gt(m), uc.FULL) for m in models]
    dl1 = Rectifier.fit_linear(cams[0], Ra, cams[1], Rb, dst, alpha=1.0)
    lo, hi = [], []
    for (m, K, size), R in zip(cams, (Ra, Rb)):
        # the fit's own samples: the corners and 64 points inside every edge
        s = np.arange(0, 66) / 65.0
        w1, h1 = size[0] - 1.0, size[1] - 1.0
        border = np.concatenate([np.stack([0 * s, s * h1], 1), np.stack([0 * s + w1, s * h1], 1), np.stack([s * w1, 0 * s], 1), np.stack([s * w1, 0 * s + h1], 1)])
        p, ok = host_points(m, K, dl1, R, border)
        # (kb4's corners lie 84 degrees off its axis: turned by the rig's few degrees some have no pinhole image, and the fit drops them)
        assert ok.all() or (m == "kb4" and ok.sum() > 200)
        lo.append(p[ok].min(0)); hi.append(p[ok].max(0))
    lo, hi = np.min(lo, 0), np.max(hi, 0)
    assert lo[0] >= -1e-6 and lo[1] >= -1e-6 and hi[0] <= dst[0] - 1 + 1e-6 and hi[1] <= dst[1] - 1 + 1e-6, (lo, hi)
    # the union fills the destination: its bounding box touches all four sides
    assert abs(lo[0]) <= 1e-6 and abs(lo[1]) <= 1e-6 and abs(hi[0] - (dst[0] - 1)) <= 1e-6 and abs(hi[1] - (dst[1] - 1)) <= 1e-6
    dl0 = Rectifier.fit_linear(cams[0], Ra, cams[1], Rb, dst, alpha=0.0)
    dlh = Rectifier.fit_linear(cams[0], Ra, cams[1], Rb, dst, alpha=0.5)
    np.testing.assert_array_less(dl1[:2], dlh[:2]); np.testing.assert_array_less(dlh[:2], dl0[:2])


def test_stereo_fit_refuses_an_empty_intersection():
    """two cameras looking 120 degrees apart share no rectangle"""
    K = uc.gt("poly3")
    cam = ("poly3", K, uc.FULL)
    out = np.zeros(4)
    Ra, Rb = uc.rotation((0.0, 60.0, 0.0)), uc.rotation((0.0, -60.0, 0.0))
    st = lib.load().vc_stereo_fit_linear(2, _p(K), 7, 640, 480, _p(Ra), 2, _p(K), 7, 640, 480, _p(Rb), 163, 121, C.c_double(0.0), _p(out))
    assert st == -6
    with pytest.raises(lib.VicalibError):
        Rectifier.fit_linear(cam, Ra, cam, Rb, (163, 121))
    assert lib.load().vc_stereo_fit_linear(2, _p(K), 7, 640, 480, _p(Ra), 2, _p(K), 6, 640, 480, _p(Rb), 163, 121, C.c_double(0.0), _p(out)) == -2


def test_undistort_fit_linear_returns_the_bits_it_did_before_the_fit_was_shared():
    with open(os.path.join(HERE, "golden", "undistort_fit_linear.json")) as f:
        cases = json.load(f)["cases"]
    assert len(cases) == 12
    for c in cases:
        K = np.array([float.fromhex(x) for x in c["params"]])
        got = lib.Undistorter.fit_linear(c["model"], K, c["src"], c["dst"], alpha=c["alpha"])
        assert c["status"] == 0 and [float(x).hex() for x in got] == c["dst_linear"], (c["model"], c["alpha"])


def test_stereo_fit_of_one_camera_twice_is_the_single_camera_fit():
    K = uc.gt("kb4")
    cam = ("kb4", K, uc.FULL)
    for alpha in (0.0, 0.5, 1.0):
        one = lib.Undistorter.fit_linear("kb4", K, uc.FULL, (163, 121), alpha=alpha)
        two = Rectifier.fit_linear(cam, np.eye(3), cam, np.eye(3), (163, 121), alpha=alpha)
        assert np.array_equal(one, two)


# ---------------------------------------------------------------------------------------------------------------- the matcher
def test_match_tiles_against_intersect1d():
    prob = synth.generate(synth.Config(models=("fov", "kb4", "poly3"), n_frames=6, pixel_sigma=0.0))
    tiles = [list(t) for t in prob.tiles]
    # frame 2: camera 2 does not see the target; frame 4: cameras 0 and 2 share no corner; every view in an order of its own
    tiles = [t for t in tiles if not (t[0] == 2 and t[1] == 2)]
    rng = np.random.default_rng(9)
    for t in tiles:
        if t[0] == 4 and t[1] in (0, 2):
            keep = (t[2] % 2 == 0) if t[1] == 0 else (t[2] % 2 == 1)
            t[2], t[3] = t[2][keep], t[3][keep]
        order = rng.permutation(len(t[2]))
        t[2], t[3] = t[2][order], t[3][order]
    tf = np.array([t[0] for t in tiles], dtype=np.int32); tc = np.array([t[1] for t in tiles], dtype=np.int32)
    off = np.concatenate([[0], np.cumsum([len(t[2]) for t in tiles])]).astype(np.int64)
    ids = np.concatenate([t[2] for t in tiles]).astype(np.int32)
    frames, foff, pa, pb = Rectifier.match_tiles(tf, tc, off, ids, 0, 2)
    assert list(frames) == [0, 1, 3, 4, 5] and foff[0] == 0 and foff[-1] == len(pa) == len(pb)
    k = 0
    for f in frames:
        ta = next(i for i, t in enumerate(tiles) if t[0] == f and t[1] == 0); tb = next(i for i, t in enumerate(tiles) if t[0] == f and t[1] == 2)
        common, ia, ib = np.intersect1d(tiles[ta][2], tiles[tb][2], return_indices=True)
        s = slice(foff[k], foff[k + 1])
        assert np.array_equal(pa[s], off[ta] + ia) and np.array_equal(pb[s], off[tb] + ib), f
        assert np.array_equal(ids[pa[s]], common) and np.array_equal(ids[pb[s]], common)
        assert (len(common) == 0) == (f == 4)
        k += 1
    assert len(pa) > 500
    # the fill call refuses arrays that are too small; a camera matched with itself is an argument error
    L = lib.load()
    nf, n = C.c_int(len(frames)), C.c_longlong(len(pa) - 1)
    st = L.vc_match_tiles(len(tf), _p(tf), _p(tc), _p(off), _p(ids), 0, 2, C.byref(nf), C.byref(n), _p(frames), _p(foff), _p(pa.copy()), _p(pb.copy()))
    assert st == -2 and n.value == len(pa)
    assert L.vc_match_tiles(len(tf), _p(tf), _p(tc), _p(off), _p(ids), 1, 1, C.byref(nf), C.byref(n), None, None, None, None) == -2


# ---------------------------------------------------------------------------------------------------------------- the check's arithmetic
def test_host_rigid_rotation_against_kabsch():
    rng = np.random.default_rng(2)
    for n in (3, 4, 50):
        P = rng.normal(size=(n, 3)) * [0.1, 0.05, 0.01] if n > 3 else rng.normal(size=(n, 3))
        Rt = uc.rotation(tuple(rng.uniform(-170, 170, 3)))
        X = P @ Rt.T + rng.normal(size=(n, 3)) * 1e-3 + [1.0, -2.0, 0.5]
        p, x = P - P.mean(0), X - X.mean(0)
        R = np.zeros((3, 3))
        _harness().vrh_rigid_rotation(_p(np.ascontiguousarray(p.T @ x)), _p(R))
        assert np.abs(R @ R.T - np.eye(3)).max() <= 1e-14 and np.linalg.det(R) > 0
        got = np.sqrt(np.sum((p @ R.T - x) ** 2) / n)
        want = rc.kabsch_rms(P, X)
        assert abs(got - want) <= 1e-9 * want + 1e-12, (n, got, want)


@pytest.mark.parametrize("models", rc.MODEL_PAIRS)
def test_host_check_exact_data(models):
    c = rc.check_case(models, 0.0)
    out, Ra = host_check(c)
    rc.check_exact(c, out, Ra)
    rc.check_frame_rows(c, out)


@pytest.mark.parametrize("models", rc.MODEL_PAIRS)
def test_host_check_against_numpy(models):
    c = rc.check_case(models, 0.1)
    out, _ = host_check(c)
    rc.check_pairs_against_reference(out, *rc.reference("noisy", models))
    rc.check_frame_rows(c, out)
    rms_dv = np.sqrt(out["sum_dv2"][5:] / out["count"][5:])
    assert 0.08 < rms_dv.min() and rms_dv.max() < 0.25 and 1e-4 < out["rigid_rms"][5:].min() and out["rigid_rms"][5:].max() < 2e-3      # the noise is there
    # without target points: no rigid fit, everything else the same bits
    bare, _ = host_check(c, with_target=False)
    assert np.isnan(bare["rigid_rms"]).all() and np.array_equal(bare["pairs"], out["pairs"]) and np.array_equal(bare["sum_dv2"], out["sum_dv2"])


@pytest.mark.parametrize("name", ["beyond", "swapped"])
def test_host_check_invalid_pairs(name):
    c = rc.beyond_case() if name == "beyond" else rc.swapped_case()
    out, _ = host_check(c)
    ref_pairs, ref_bad = rc.reference(name)
    assert np.array_equal(np.nonzero(ref_bad)[0], c.bad)
    rc.check_pairs_against_reference(out, ref_pairs, ref_bad)
    rc.check_frame_rows(c, out)
    k = int(np.searchsorted(c.frame_off, c.bad[0], side="right") - 1)
    assert out["count"][k] == 65 - 1 and out["n_invalid"][k] == 1 and out["n_invalid"].sum() == 1


# ---------------------------------------------------------------------------------------------------------------- CLI, device
def test_cli_lists_the_rectify_flags():
    r = subprocess.run([BIN, "-help"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0
    for flag in ("-rectify_dir", "-rectify_cams", "-rectify_alpha"):
        assert flag + " " in r.stdout, flag
    r = subprocess.run([BIN, "-rectify_dir", "out", "-rectify_cams", "0,1", "-rectify_alpha", "0.5", "-cam", "detections:///does/not/exist.csv"], capture_output=True,
                       text=True, timeout=60)
    assert r.returncode == 1 and "cannot open" in r.stderr and "unknown command line flag" not in r.stderr


def test_no_cpu_fallback_without_device():
    if _have_gpu():
        pytest.skip("GPU present")
    L = lib.load()
    Ta, Tb = rc.generator_rig(("fov", "fov"))
    K = uc.gt("fov"); h = C.c_void_p()
    args = (0, K, 5, 640, 480, Ta, 0, K, 5, 640, 480, Tb)
    conv = lambda a: [_p(x) if isinstance(x, np.ndarray) else x for x in a]      # noqa: E731
    assert L.vc_rectifier_create(0, *conv(args), _p(rc.DST_LINEAR), 640, 480, C.c_double(0.0), 0, C.byref(h)) == -1      # VC_ERR_NO_DEVICE
    assert L.vc_rectifier_create(0, *conv(args), None, 640, 480, C.c_double(0.0), 0, C.byref(h)) == -1                   # ... after the fit
    assert not h.value
    with pytest.raises(lib.VicalibError):
        Rectifier(("fov", K, (640, 480), Ta), ("fov", K, (640, 480), Tb))


def test_arguments_are_checked_before_the_device():
    L = lib.load()
    Ta, Tb = rc.generator_rig(("fov", "fov"))
    K = uc.gt("fov"); h = C.c_void_p()
    create = lambda nk, Tb_, dl, alpha, fill: L.vc_rectifier_create(0, 0, _p(K), 5, 640, 480, _p(Ta), 0, _p(K), nk, 640, 480, _p(Tb_), dl, 640, 480,      # noqa: E731
                                                                     C.c_double(alpha), fill, C.byref(h))
    assert create(4, Tb, None, 0.0, 0) == -2 and create(5, Tb, None, 1.5, 0) == -2 and create(5, Tb, None, 0.0, 256) == -2
    assert create(5, Ta.copy(), None, 0.0, 0) == -6                                          # coincident centres
    assert create(5, rc.vertical_rig()[1], None, 0.0, 0) == -7                               # a vertical pair (a is at the origin in both rigs)
    out = np.zeros(4)
    assert L.vc_rectify_check(None, 1, _p(np.zeros(2, dtype=np.int64)), None, None, None, None, None, None, None, None, None, None, None, None, None) == -2
    assert L.vc_rectifier_get(None, None, None, _p(out), None, None, None, None) == -2 and L.vc_time_rectify_check(None, 1, _p(out)) == -2
    assert not L.vc_rectifier_side(None, 0)
