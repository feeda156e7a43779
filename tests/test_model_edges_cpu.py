"""The camera models at their branch points, host side: the mpmath reference of tests/golden/model_edges.json against the host build
of vc_math.hpp (the existing harness: hh_project, hh_tile_gram, hh_frame_blocks, hh_cam_block), the reference's generator against the
oracle on a generic board (it restates the same operation, not a private one), and the host build's largest deviations per quantity --
the figures the device bounds of test_model_edges_gpu.py stand next to in DESIGN.md section 5."""
import ctypes as C
import importlib.util
import os
import numpy as np
import pytest

import model_edges_cases as mc
import oracle_lib as ol
from test_device_math_cpu import hh
from vicalib_amd import synth

HERE = os.path.dirname(os.path.abspath(__file__))
d = ol._d
_gen = None


def generator():
    global _gen
    if _gen is None:
        pytest.importorskip("mpmath")
        spec = importlib.util.spec_from_file_location("make_golden_model_edges", os.path.join(HERE, "golden", "make_golden_model_edges.py"))
        _gen = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(_gen)
    return _gen


def _split_w(cam, dev):
    """(entries that do not involve fov's w column, entries that do)"""
    _, col = mc.w_factor(cam)
    m = np.zeros(dev.shape, dtype=bool)
    if col >= 0:
        m[..., col] = True
        if dev.ndim == 2 and dev.shape[0] == dev.shape[1]:
            m[col, :] = True
    return dev[~m], dev[m]


def host_points(cam, mx):
    """hh_project over the camera's points against the fixture; returns the cases out of bounds"""
    H = hh(); bad = []
    nk = cam["nk"]; fac, _ = mc.w_factor(cam)
    for i, tag in enumerate(cam["tags"]):
        what = "%s %s" % (cam["name"], tag)
        pix = np.zeros(2); A = np.zeros((2, 3)); B = np.zeros((2, nk))
        H.hh_project(cam["model"], d(cam["p"][i]), d(cam["k"]), d(pix), d(A), d(B))
        ok = mx.add("pixel", mc.dev_pixel(pix[None, :], cam["pix"][i][None, :], cam["k"], what), mc.PIXEL_BOUND, what)
        ok &= mx.add("A", mc.dev_block(A, cam["A"][i], what), mc.BLOCK_BOUND, what)
        b, bw = _split_w(cam, mc.dev_block(B, cam["B"][i], what))
        ok &= mx.add("B", b, mc.BLOCK_BOUND, what)
        ok &= mx.add("B, fov w column", bw, min(mc.BLOCK_BOUND * fac, mc.CAP), what)
        if not ok:
            bad.append(what)
    return bad


def host_frames(cam, mx):
    """hh_tile_gram + hh_frame_blocks + hh_cam_block (flags = 4, identity poses) over the camera's two frames against the fixture"""
    H = hh(); bad = []
    nk = cam["nk"]; fac, _ = mc.w_factor(cam)
    wb = min(mc.H_BOUND * fac, mc.CAP)
    for fr in cam["frames"]:
        what = "%s frame %s" % (cam["name"], fr["tag"])
        G = np.zeros(272); Hff = np.zeros(36); g6 = np.zeros(6); Hcc = np.zeros(256); gc = np.zeros(16)
        cost = 0.5 * H.hh_tile_gram(cam["model"], d(mc.IDENTITY), d(mc.IDENTITY), d(cam["k"]), len(fr["pw"]), d(fr["pw"]), d(fr["uv"]), C.c_double(1.0), d(G))
        H.hh_frame_blocks(d(G), d(mc.IDENTITY), nk, 4, d(Hff), d(g6), None)
        H.hh_cam_block(d(G), d(mc.IDENTITY), nk, 4, d(Hcc), d(gc))
        ok = mx.add("H_pp", mc.dev_H(Hff.reshape(6, 6), fr["Hpp"], what), mc.H_BOUND, what)
        ok &= mx.add("g_p", mc.dev_g(g6, fr["gp"], np.diag(fr["Hpp"]), fr["cost"], what), mc.G_BOUND, what)
        ok &= mx.add("cost", mc.dev_cost(cost, fr["cost"], what), mc.COST_BOUND, what)
        h, hw = _split_w(cam, mc.dev_H(Hcc.reshape(16, 16)[:nk, :nk], fr["Hkk"], what))
        g, gw = _split_w(cam, mc.dev_g(gc[:nk], fr["gk"], np.diag(fr["Hkk"]), fr["cost"], what))
        ok &= mx.add("H_kk", h, mc.H_BOUND, what) & mx.add("H_kk, fov w column", hw, wb, what)
        ok &= mx.add("g_k", g, mc.G_BOUND, what) & mx.add("g_k, fov w column", gw, wb, what)
        if not ok:
            bad.append(what)
    return bad


def test_generator_reproduces_the_committed_fixture():
    gen = generator()
    assert gen.dumps(gen.build_fixture()) == open(os.path.join(HERE, "golden", "model_edges.json")).read()


def test_fixture_covers_the_case_table():
    """every branch the table names is in the fixture, on the side of its threshold it is meant to be"""
    cams = mc.cameras()
    assert sorted(set(c["model"] for c in cams)) == [0, 1, 2, 3, 4, 5]
    w = sorted(c["k"][4] for c in cams if c["model"] == 0)
    assert w == [-0.92, 0.0, 0.003, 0.00316, 0.00317, 0.92, 2.6]
    assert [c["fix_k"] for c in cams if c["model"] == 0] == [not (c["k"][4] ** 2 > 1e-5) for c in cams if c["model"] == 0]
    for c in cams:
        p = c["p"]; tags = c["tags"]
        r = np.hypot(p[:, 0], p[:, 1]) / np.where(p[:, 2] != 0.0, np.abs(p[:, 2]), 1.0)
        on = (p[:, 0] == 0.0) & (p[:, 1] == 0.0)
        assert on.sum() == 2 and len(set(p[on, 2])) == 2
        small = r[~on & (r < 3.1e-3)]
        assert small.min() <= 1e-9 * 1.01 and small.max() >= 3e-3 * 0.99
        edge = np.sqrt(1e-5)
        assert np.any((r > 0.98 * edge) & (r < 0.99 * edge)) and np.any((r > 1.01 * edge) & (r < 1.02 * edge))
        assert not np.any((r >= 0.99 * edge) & (r <= 1.01 * edge))
        for want in (0.36, 0.66, 0.99, 2.7, 86.0):
            assert np.any(np.abs(r - want) < 0.01 * want + 0.005), (c["name"], want)
        assert np.any(np.abs(p).max(axis=1) > 2.0 ** 39) and np.any((np.abs(p).max(axis=1) < 2.0 ** -39) & ~on)
        assert np.any(p[:, 2] < 0.0)
        assert ("z0" in tags) == (c["model"] == 3)
        assert np.all(p[:, 2] != 0.0) or c["model"] == 3
        for lo, hi in ((0.65, 0.67), (2.40, 2.43)):
            assert np.any(np.abs(r - lo) < 1e-9) and np.any(np.abs(r - hi) < 1e-9)
        assert np.any((p[:, 2] == -1.0) & (np.abs(r - 1e-3) < 1e-9))
        assert [f["tag"] for f in c["frames"]] == ["axis", "wide"]
        for f in c["frames"]:
            assert f["pw"].shape == (8, 3) and np.all(f["pw"][:, 2] == 1.0)
        assert np.any(np.all(c["frames"][0]["pw"][:, :2] == 0.0, axis=1))
    kat = [0.12, 0.05, 0.004, 0.40, -0.04, 0.002]
    assert list(mc.camera("rational6")["k"][4:]) == kat


@pytest.mark.parametrize("name", mc.camera_names())
def test_host_projection_matches_the_reference(name):
    mx = mc.Maxima()
    bad = host_points(mc.camera(name), mx)
    print("\n".join(mx.lines()))
    assert not bad, (bad, mx.lines())


@pytest.mark.parametrize("name", mc.camera_names())
def test_host_gram_blocks_match_the_reference(name):
    mx = mc.Maxima()
    bad = host_frames(mc.camera(name), mx)
    print("\n".join(mx.lines()))
    assert not bad, (bad, mx.lines())


def test_host_build_largest_deviations():
    """The calibration of the device bounds: the host build's largest deviation from the mpmath values per quantity over the whole table
    (printed; DESIGN.md section 5 quotes them).  The host build has neither contraction nor the Newton reciprocals: it has to stay
    inside the device bounds.  The two largest are cancellations of the inputs, not of the code: the pixel of fov at r = 2.4 lands
    16 px from the origin out of terms of 336 px (2.7e-15 on max(|pix|, 1)), and dpix/dZ at r = 86 multiplies the rounding of the
    tangential entries by r (3.9e-14 of the block's largest entry, about 4 * 1.1e-16 * 86)."""
    mx = mc.Maxima()
    for cam in mc.cameras():
        host_points(cam, mx); host_frames(cam, mx)
    print("\n".join(mx.lines()))
    assert set(mx.m) >= {"pixel", "A", "B", "B, fov w column", "H_pp", "g_p", "cost", "H_kk", "g_k", "H_kk, fov w column", "g_k, fov w column"}
    for q, (dev, rel, what) in mx.m.items():
        assert rel <= 1.0, (q, dev, rel, what)


def test_reference_generator_matches_the_oracle_on_a_generic_board():
    """The generator's residual, central-difference Jacobians, robust weights and sums against the oracle's normal equations (autodiff x
    local parameterisation, as the reference) on a synth board in general position, fov + kb4, 3 frames, 10 corners per view: frame
    blocks A, gradients gf and gs, and the cost.  The oracle is well defined there and exact to double rounding."""
    gen = generator()
    mp = gen.mp
    p = synth.generate(synth.Config(models=("fov", "kb4"), n_frames=3, seed=11))
    o = ol.Oracle()
    cams = []
    for c, m in enumerate(p.cam_model):
        o.add_camera(m, p.cam_K_init[c], p.cam_T_ck_init[c], p.cfg.width, p.cfg.height)
        cams.append((gen.MODEL_NAMES[int(m)], [mp.mpf(float(v)) for v in p.cam_K_init[c]], [mp.mpf(float(v)) for v in p.cam_T_ck_init[c]]))
    poses = []
    for n in range(3):
        o.add_frame(p.frame_T_wk_init[n], p.frame_time[n])
        poses.append([mp.mpf(float(v)) for v in p.frame_T_wk_init[n]])
    tiles = []
    for (f, c, ids, pix) in p.tiles:
        pw = np.ascontiguousarray(p.grid_points[ids[:10]]); uv = np.ascontiguousarray(pix[:10])
        o.add_observations(f, c, pw, uv)
        tiles.append((f, c, [[mp.mpf(float(v)) for v in q] for q in pw], [[mp.mpf(float(v)) for v in q] for q in uv]))
    assert len(tiles) == 6
    o.set_options(calibrate_imu=False)
    o.prepare(vis_mult=1)
    lin = o.linearize(); lay = o.layout()
    Hf, gf, Hc, gc, cost = gen.normal_equations(cams, poses, tiles)
    cost = float(cost)
    assert abs(lin["cost"] - cost) <= 1e-12 * cost
    for f in range(3):
        ref = np.array([[float(v) for v in row] for row in Hf[f]]); g = np.array([float(v) for v in gf[f]])
        assert mc.dev_H(lin["A"][f, :6, :6], ref, "A").max() <= 1e-10
        assert mc.dev_g(lin["gf"][f, :6], g, np.diag(ref), cost, "gf").max() <= 1e-10
    seen = 0
    for c in range(2):
        nk = len(cams[c][1])
        ref = np.array([[float(v) for v in row] for row in Hc[c]]); g = np.array([float(v) for v in gc[c]])
        for off, lo, n in ((lay["cam"][c][0], 0, 3), (lay["cam"][c][1], 3, 3), (lay["cam"][c][2], 6, nk)):
            if off < 0:
                continue
            seen += n
            assert mc.dev_g(lin["gs"][off:off + n], g[lo:lo + n], np.diag(ref)[lo:lo + n], cost, "gs").max() <= 1e-10
            assert mc.dev_H(lin["Hss"][off:off + n, off:off + n], ref[lo:lo + n, lo:lo + n], "Hss").max() <= 1e-10
    assert seen == lay["D"] == 5 + 8 + 6
