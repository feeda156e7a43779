"""The predicted centre bias of a dot on the device (vc_dot_bias_batch: one wavefront per observation, boundary sample i in lane i) against the numpy
reference (tests/dot_bias_ref.py), on the batches of tests/dot_bias_cases.py with that file's checks: statuses exactly, bias and radius_px
within 100 times the spread between the reference's two routes, the outputs of a refused observation untouched.  Determinism is compared on
the raw bytes: a fixed reduction order promises the same bits for an observation alone, among others and on a second run.

Measured (MI355X): see DESIGN 4.20."""
import ctypes as C

import numpy as np
import pytest

import dot_bias_cases as dc
import vicalib_amd.lib as lib

pytestmark = pytest.mark.gpu
BAD_ARG = -2
KEYS = ("status", "bias", "radius_px")


def _run(arrays):
    return lib.dot_bias_batch(*arrays, out=dc.prefilled(len(arrays[5])))


@pytest.fixture(scope="module")
def runs():
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = _run(dc.batch_arrays(dc.group(name)))
        return cache[name]
    return get


@pytest.mark.parametrize("name", dc.GROUPS)
def test_batch_matches_the_reference(runs, name):
    dc.check(name, runs(name), label=" (device)")


@pytest.mark.parametrize("n", dc.PREFIXES)
def test_every_batch_shape(runs, n):
    """0 observations, 1 (a lone wave), 3, 4 (a full workgroup), 5 (a workgroup and one wave), 257 (65 workgroups, the last with one wave), over
    views of uneven size with empty ones among them; every shape against the reference and bit for bit against the rows of the whole batch"""
    arrays, rows = dc.prefix(n)
    got = _run(arrays)
    dc.check("models", got, label=" (device, %d observations)" % n, rows=rows)
    for key in KEYS:
        assert got[key].tobytes() == runs("models")[key][:n].tobytes(), (n, key)


def test_an_observation_gives_the_same_bits_alone_and_again(runs):
    full = runs("models")
    again = _run(dc.batch_arrays(dc.group("models")))
    for key in KEYS:
        assert again[key].tobytes() == full[key].tobytes(), key
    g = dc.group("models")
    for k in range(257):
        alone = _run(dc.batch_arrays(g, keep=[k]))
        for key in KEYS:
            assert alone[key].tobytes() == full[key][k:k + 1].tobytes(), (k, key)


def test_statuses(runs):
    assert runs("status")["status"].tolist() == dc.group("status")["expect"]
    assert (runs("sizes")["status"] == 0).all() and np.all(runs("sizes")["bias"][[0, 4, 8]] == 0.0) and np.all(runs("sizes")["radius_px"][[0, 4, 8]] == 0.0)


def test_argument_errors_come_before_the_device():
    L = lib.load()
    m, K, T, off, pw, rad = dc.c_arrays(*dc.batch_arrays(dc.group("axis")))
    bias, rpx, status = np.full((6, 2), dc.FILL), np.full(6, dc.FILL), np.full(6, -1, dtype=np.int32)
    call = lambda n=6, model=m, o=off, radius=rad, b=bias: L.vc_dot_bias_batch(0, n, dc._p(model), dc._p(K), dc._p(T), dc._p(o), dc._p(pw), dc._p(radius),
                                                                             dc._p(b) if b is not None else None, dc._p(rpx), dc._p(status))
    assert call(n=-1) == BAD_ARG and call(b=None) == BAD_ARG
    assert call(model=np.array([0, 1, 2, 3, 4, 9], dtype=np.int32)) == BAD_ARG
    assert call(o=np.array([0, 1, 2, 3, 2, 5, 6], dtype=np.int32)) == BAD_ARG
    bad = rad.copy(); bad[4] = -1e-9
    assert call(radius=bad) == BAD_ARG
    bad[4] = np.nan
    assert call(radius=bad) == BAD_ARG
    assert np.all(bias == dc.FILL) and np.all(rpx == dc.FILL) and np.all(status == -1)          # nothing was written
    assert call() == 0 and (status == 0).all()


def test_timing_hook_runs():
    assert lib.time_dot_bias_batch(*dc.batch_arrays(dc.group("models")), reps=3) > 0.0
