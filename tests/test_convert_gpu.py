"""Converting a calibrated camera to another camera model on the device (vc_convert*, vicalib_amd/csrc/vc_convert.hip): the kernels against the
numpy reference and the checks of tests/convert_cases.py (the ones tests/test_convert_cpu.py applies to the host build of the same arithmetic),
their determinism, the lattice of exactly one workgroup, a calibrator's camera, argument errors of a run, and the command line."""
import os
import re
import subprocess

import numpy as np
import pytest

import compare_cases as cc
import convert_cases as cv
import rectify_cases as rc
import undistort_cases as uc
import vicalib_amd.lib as lib
from vicalib_amd import synth
from vicalib_amd.lib import Converter, ViCalibrator

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "vicalib_amd", "vicalib")


def converter(c):
    return Converter(c.a, c.mb, cv.SIZE, c.grid)


def run_on(cvt, c):
    return cvt.run(c.fit_radius, c.max_iters, c.user_start, c.free_mask)


def same_bits(a, b):
    return all(np.array_equal(a[k], b[k]) for k in ("K", "status", "iterations", "n_fit", "n_left_out", "cost0", "cost", "max_err", "worst"))


@pytest.mark.parametrize("name", cv.case_names())
def test_cases_against_numpy(name):
    """checks 1 - 5, then the same bits from a second run of the handle and from a second handle"""
    c = cv.case(name)
    cvt = converter(c)

    def compare(case, K):
        cmp = cvt.comparer()
        cmp.run(0.0)
        s = cmp.summary()
        assert s["invalid"] == 0
        return s
    first = cv.check_case(name, lambda case: run_on(cvt, case), compare)
    assert same_bits(first, run_on(cvt, c)) and same_bits(first, run_on(converter(c), c))


def test_one_workgroup_lattice():
    """64 x 16 = 1024 samples: exactly one full workgroup of the sweeps"""
    c = cv.case("same-poly3-one-workgroup")
    ref = cv.reference(c.name)
    out = run_on(converter(c), c)
    assert out["n_fit"] == 1024
    cv.check_cost(ref, out)
    cv.check_zero(ref, out)


def test_readers_before_a_run_arguments_and_timing():
    c = cv.case("rational6-poly3")
    cvt = converter(c)
    for read in (cvt.get, cvt.comparer, cvt.time):
        with pytest.raises(lib.VicalibError, match="BAD_ARG"):
            read()
    bad = c.start.copy(); bad[5] = np.nan
    for kw in (dict(fit_radius=0.0), dict(fit_radius=-1.0), dict(fit_radius=float("nan")), dict(start=bad), dict(free_mask=1 << 7)):
        with pytest.raises(lib.VicalibError, match="BAD_ARG"):
            cvt.run(**kw)
    with pytest.raises(lib.VicalibError, match="BAD_ARG"):
        cvt.get()                                                # a refused run leaves nothing to read
    capped = cvt.run(1.0, 2)
    assert capped["status"] == 1 and capped["iterations"] == 2 and capped["cost"] < capped["cost0"]
    full = cvt.run(1.0)
    # another fit radius on the same handle: the fit set is counted again
    half = cvt.run(0.5)
    rho = cc.lattice(cv.SIZE, c.grid)[1]
    assert half["n_fit"] == (rho <= 0.5).sum() and full["n_fit"] == len(rho) and half["cost"] < full["cost"]
    assert (cvt.time(2) > 0).all()
    # 2 x 2: eight residuals for the ten parameters of rational6
    tiny = Converter(c.a, "rational6", cv.SIZE, (2, 2))
    with pytest.raises(lib.VicalibError, match="NUMERIC"):
        tiny.run(1.0)
    assert tiny.run(1.0, 0, None, 0xf)["n_fit"] == 4


def test_for_camera_of_a_calibrator():
    """a calibrator that only had a camera added: the source is that camera"""
    c = cv.case("poly3-kb4")
    cal = ViCalibrator(0)
    cal.AddCamera(synth.MODEL_IDS[c.a[0]], c.a[1], rc.IDENTITY_POSE, cv.SIZE[0], cv.SIZE[1])
    mine = Converter.for_camera(cal, 0, c.mb, c.grid)
    assert same_bits(mine.run(1.0), converter(c).run(1.0))
    with pytest.raises(lib.VicalibError, match="BAD_ARG"):
        Converter.for_camera(cal, 1, c.mb, c.grid)


# ---------------------------------------------------------------------------------------------------------------- the command line
def _cameras(text):
    """[(type, params, T_wc entries)] of a rig file, every number as the file's text"""
    cams = []
    for block in re.findall(r"<camera>(.*?)</camera>", text, re.S):
        kind = re.search(r'type="(.*?)"', block).group(1)
        params = np.array([float(x) for x in re.search(r"<params> \[(.*?)\] </params>", block).group(1).split(";")])
        pose = [x.strip() for x in re.split(r"[;,]", re.search(r"<T_wc> \[(.*?)\] </T_wc>", block, re.S).group(1))]
        size = (int(re.search(r"<width> (\d+) </width>", block).group(1)), int(re.search(r"<height> (\d+) </height>", block).group(1)))
        cams.append((kind, params, pose, size))
    return cams


def test_cli_convert_models(tmp_path):
    """a two-camera rig converted by the tool, one target model per camera: the written rig has the original poses and sizes, camera 0 (poly3 to
    kb4) passes check 2 and camera 1 (kb4 to kb4) check 3; with -compare_dir the comparison of the original against the converted cameras"""
    Ta, Tb = rc.hand_rig()
    a, out, cmp_dir = tmp_path / "a.xml", tmp_path / "converted.xml", tmp_path / "cmp"
    a.write_text(cc.rig_xml([("poly3", uc.gt("poly3"), Ta), ("kb4", uc.gt("kb4"), Tb)]))
    r = subprocess.run([BIN, "-convert_models", str(a), "-convert_to", "kb4,kb4", "-convert_output", str(out), "-convert_grid", "%dx%d" % cv.GRID,
                        "-compare_dir", str(cmp_dir)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    before, after = _cameras(a.read_text()), _cameras(out.read_text())
    assert len(after) == 2
    for (k0, p0, pose0, size0), (k1, p1, pose1, size1) in zip(before, after):
        assert k1 == cc.XML_TYPES["kb4"] and size1 == size0 == cv.SIZE
        assert [float(x) for x in pose1] == [float(x) for x in pose0]          # the original poses, bit-equal
    for cam, name in enumerate(("poly3-kb4", "same-kb4")):
        ref = cv.reference(name)
        K = after[cam][1]
        d = ref.d(K)
        stats = dict(K=K, status=0, iterations=0, cost0=np.inf, cost=0.5 * float(np.sum(d ** 2)), max_err=float(np.sqrt(np.sum(d ** 2, axis=1)).max()))
        line = [ln for ln in r.stdout.splitlines() if ln.startswith("camera %d:" % cam) and "converted" in ln]
        assert len(line) == 1 and "status 0" in line[0], r.stdout[-1000:]
        if ref.c.e_opt is None:
            cv.check_zero(ref, stats)
        else:
            cv.check_optimal(ref, stats)
    rows = open(cmp_dir / "compare_summary.csv").read().splitlines()
    assert rows[1].split(",")[:3] == ["0", "poly3", "kb4"] and rows[2].split(",")[:3] == ["1", "kb4", "kb4"]
    assert abs(float(rows[1].split(",")[14]) - np.sqrt(2.0 * stats_cost(cv.reference("poly3-kb4"), after[0][1]) / 2173)) <= 1e-7


def stats_cost(ref, K):
    return 0.5 * ref.E(K)


def test_cli_convert_to_behind_a_calibration(tmp_path):
    """a small vision-only solve with -convert_to: the rig just written, converted -- the same poses and sizes, kb4 parameters that a Converter
    gives for the camera the tool wrote into cameras.xml (its parameters are printed with 17 digits)"""
    prob = synth.generate(synth.Config(models=("poly3",), n_frames=12, seed=3))
    files, _ = synth.write_dataset(prob, str(tmp_path))
    result, out = tmp_path / "cameras.xml", tmp_path / "converted.xml"
    r = subprocess.run([BIN, "-cam", "detections://" + ",".join(files), "-models", "poly3", "-nocalibrate_imu", "-output", str(result), "-convert_to", "kb4",
                        "-convert_output", str(out)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    (k0, p0, pose0, size0), = _cameras(result.read_text())
    (k1, p1, pose1, size1), = _cameras(out.read_text())
    assert k0 == cc.XML_TYPES["poly3"] and k1 == cc.XML_TYPES["kb4"] and pose1 == pose0 and size1 == size0
    want = Converter(("poly3", p0), "kb4", size0).run(1.0, 200)
    assert np.array_equal(p1, want["K"]) and want["status"] == 0
    assert "camera 0: poly3 converted to kb4: status 0" in r.stdout
