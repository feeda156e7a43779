"""What of the residual report needs no device: the command line's flags and the binning of the error maps, compiled for the host."""
import ctypes as C
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
BIN = os.path.join(ROOT, "vicalib_amd", "vicalib")


def _run(args):
    return subprocess.run([BIN] + args, capture_output=True, text=True, timeout=120)


def test_help_lists_the_report_flags():
    h = _run(["--help"])
    assert h.returncode == 0
    for flag in ("-report_dir", "-report_bins", "-report_worst"):
        assert flag + " " in h.stdout, flag
    line = [ln for ln in h.stdout.splitlines() if ln.lstrip().startswith("-output_conics ")][0]
    assert "-report_dir" in line                     # where the residuals of the echoed detections come from


def test_report_bins_are_checked_before_anything_is_read():
    for bad in ("0x4", "33x1", "abc", "16x", "x12", "16x12x3", "4x-1"):
        r = _run(["-cam", "detections:///does/not/exist.csv", "-report_bins", bad])
        assert r.returncode == 1 and "report_bins" in r.stderr and "cannot open" not in r.stderr, bad
    for good in ("16x12", "1x1", "32x32"):
        r = _run(["-cam", "detections:///does/not/exist.csv", "-report_bins", good])
        assert r.returncode == 1 and "cannot open" in r.stderr, good           # got as far as the detections
    r = _run(["-cam", "detections:///does/not/exist.csv", "-report_worst", "abc"])
    assert r.returncode == 1 and "illegal value" in r.stderr


def _harness():
    src = os.path.join(HERE, "host_harness", "report_harness.cpp")
    so = os.path.join(HERE, "host_harness", "libvc_report_harness.so")
    dep = os.path.join(ROOT, "vicalib_amd", "csrc", "vc_report_bins.hpp")
    if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(src), os.path.getmtime(dep)):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-o", so, src])
    return C.CDLL(so)


def test_binning_matches_its_numpy_statement():
    """ix = clamp(int(floor(u * bins / extent)), 0, bins - 1): the device function, built for the host, against numpy on pixels that sit
    on cell edges, just beside them, outside the image and nowhere (NaN, infinities)."""
    L = _harness()
    rng = np.random.default_rng(4)
    for bins, extent in [(16, 640), (12, 480), (1, 640), (32, 641), (7, 1280), (32, 3)]:
        edges = np.arange(bins + 1) * extent / bins
        x = np.concatenate([rng.uniform(-50, extent + 50, 4000), edges, np.nextafter(edges, -np.inf), np.nextafter(edges, np.inf),
                            [np.nan, np.inf, -np.inf, 1e300, -1e300, 0.0, -0.0, extent]])
        out = np.zeros(len(x), dtype=np.int32)
        L.vcr_cells(np.ascontiguousarray(x).ctypes.data_as(C.c_void_p), len(x), bins, extent, out.ctypes.data_as(C.c_void_p))
        with np.errstate(invalid="ignore"):
            want = np.floor(x * bins / extent)
        want = np.where(np.isnan(want), 0.0, want)            # a NaN pixel goes to cell 0
        want = np.clip(want, 0, bins - 1).astype(np.int32)
        np.testing.assert_array_equal(out, want)
        assert out.min() >= 0 and out.max() <= bins - 1
