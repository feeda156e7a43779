"""Conditions on the inputs of tests/test_detect_edges_gpu.py, checked on the numpy restatement alone (no GPU): a GPU test built on an input
that does not do what it is meant to do would pass vacuously.  Every case here is one the GPU file runs through the kernels."""
import numpy as np
import pytest

import detect_cases as dc
from detect_cases import vco_detect


def _label4_components(fg, w, h):
    """What components() returns, derived from the restatement's own labelling."""
    lab = vco_detect.label4(fg)
    boxes = []
    for L in np.unique(lab[lab >= 0]):                   # (ascending label = ascending smallest pixel index)
        ys, xs = np.nonzero(lab == L)
        assert L == (ys * w + xs).min()
        x0, y0, x1, y1 = xs.min(), ys.min(), xs.max(), ys.max()
        if x0 - 2 >= 1 and y0 - 2 >= 1 and x1 + 1 + 2 <= w - 1 and y1 + 1 + 2 <= h - 1:
            boxes.append((x0, y0, x1, y1))
    return np.array(boxes, dtype=np.int64).reshape(-1, 4)


@pytest.mark.parametrize("name", list(dc.STRESS))
def test_both_labellings_agree_on_the_stress_images(name):
    """scipy's labelling and label4 (written as the device's own design): same number of components, same boxes, same order.  The
    image thresholds to exactly the mask it was drawn from, and no candidate's fit is singular (the device leaves such a candidate
    out, which is not what these images test)."""
    mask = dc.stress_mask(name)
    h, w = mask.shape
    img = dc.mask_image(mask)
    p = dc.STRESS_PARAMS
    assert int(w / p["at_window_ratio"]) >= 2
    np.testing.assert_array_equal(vco_detect.adaptive_threshold(img, p["at_threshold"], p["at_window_ratio"]), mask)
    boxes, area = dc.components(mask, w, h)
    np.testing.assert_array_equal(boxes, _label4_components(mask, w, h))
    assert dc.passing(boxes, area, p["min_area"], p["min_density"], p["min_aspect"]).all() and len(boxes) <= 4096
    for b in boxes:
        M, used = dc.normal_matrix(img, b)
        assert used >= 5 and np.linalg.cond(M) < 1e12, (b, used)
    if name == "spiral":
        assert len(boxes) == 1 and area[0] == mask.sum() > 4000 and boxes[0][2] - boxes[0][0] == 95      # one component through 3 x 3 tiles
    elif name == "serpentine":
        assert len(boxes) == 1 and area[0] == 527 and tuple(boxes[0]) == (32, 32, 63, 62)                 # inside the tile [32, 64)^2
    else:
        assert len(boxes) >= 100 and area.max() >= 50
        crossing = (boxes[:, 0] // 32 != boxes[:, 2] // 32) | (boxes[:, 1] // 32 != boxes[:, 3] // 32)
        assert crossing.sum() >= 10                                                                        # pieces to join across tile edges


@pytest.mark.parametrize("name", list(dc.PARAM_CASES))
def test_every_parameter_case_changes_the_result(name):
    """A parameter that the device dropped, swapped or compared the wrong way round must show: at the case's values the restatement
    finds other dots than at the defaults on the same image."""
    _, _, b0 = dc.param_reference(None)
    _, _, b = dc.param_reference(name)
    assert len(b0) >= 50
    assert b.shape != b0.shape or not np.array_equal(b, b0)


def test_parameter_cases_cover_both_directions():
    n0 = len(dc.param_reference(None)[0])
    n = {k: len(dc.param_reference(k)[0]) for k in dc.PARAM_CASES}
    assert n["min_aspect_0.21"] < n0 < n["min_aspect_0.1"]
    assert n["min_density_0.9"] < n0 < n["min_density_0.3"]
    assert n["at_threshold_0.12"] < n0 < n["at_threshold_0.95"]
    assert n["min_area_5"] == n0 - 1 and n["at_window_ratio_1000"] == 0 < n["at_window_ratio_640"] < n0
    assert set(dc.PARAM_CASES["all_six_inverted"]) == set(dc.DEFAULTS) | {"black_on_white"}
    assert all(dc.PARAM_CASES["all_six_inverted"][k] != v for k, v in dc.DEFAULTS.items())


@pytest.mark.parametrize("w,h", dc.SIZES)
def test_the_restatement_finds_every_blob_of_a_size_case(w, h):
    img, p, at = dc.size_case(w, h)
    rad = int(w / p["at_window_ratio"])
    assert img.shape == (h, w) and rad >= 2 and len(at) >= 1
    cen, _, boxes = dc.reference(img, p)
    np.testing.assert_array_equal(boxes, [(x, y, x + 1, y + 1) for x, y in at])
    xs = sorted({x for x, _ in at})
    # a blob alone in its grown box has its centre in the middle; 509 and 513 are in each other's boxes and pull by 0.39 px
    alone = np.array([not (w >= 518 and x in (509, 513)) for x, _ in at])
    np.testing.assert_allclose(cen[alone], (np.array(at) + 0.5)[alone], rtol=0, atol=1e-9)
    assert np.abs(cen - (np.array(at) + 0.5)).max() < 0.5
    if w >= 512:
        assert xs[-1] + 1 + rad + 1 >= w                  # the last blob's window ends at the last entry of the row's running sum
        assert any(x > 512 for x in xs) == (w >= 518)     # a blob in the second round wherever one fits
    if w >= 1024:
        assert {509, 513} <= set(xs) and xs[-1] > 1016


def test_the_large_image_wraps_inside_the_patch():
    """The exact integral image is below 2^32 at the patch's top-left corner and above it at its bottom-right corner: the device's 32-bit
    running sums wrap inside the patch, in rows that hold dots.  The crop that serves as reference sees every dot as the large image does."""
    img = dc.big_image()
    assert img.shape == (dc.BIG_H, dc.BIG_W) and img.size <= 2 ** 26
    s_tl = int(img[:dc.BIG_Y, :dc.BIG_X].sum(dtype=np.int64))
    s_br = int(img[:dc.BIG_Y + dc.BIG_PATCH, :dc.BIG_X + dc.BIG_PATCH].sum(dtype=np.int64))
    assert s_tl < 2 ** 32 < s_br
    crop, (ox, oy) = dc.big_crop()
    np.testing.assert_array_equal(crop, img[oy:, ox:])
    rad = dc.BIG_RAD
    assert int(dc.BIG_W / dc.ratio_for(dc.BIG_W, rad)) == int(dc.BIG_CROP / dc.ratio_for(dc.BIG_CROP, rad)) == rad
    cen, _, boxes = dc.reference(crop, dc.params(at_window_ratio=dc.ratio_for(dc.BIG_CROP, rad)))
    assert len(cen) >= 20
    assert boxes[:, 0].min() > 2 * rad + 1 + 2 and boxes[:, 1].min() > 2 * rad + 1 + 2
    # the wrap falls among the dots: some boxes begin below 2^32, some end above it (two corners per box, not the whole table)
    below = [int(img[:oy + b[1], :ox + b[0]].sum(dtype=np.int64)) < 2 ** 32 for b in boxes]
    above = [int(img[:oy + b[3] + 1, :ox + b[2] + 1].sum(dtype=np.int64)) > 2 ** 32 for b in boxes]
    assert any(below) and any(above)


def test_the_window_rule_at_its_edge():
    assert dc.window_fits(dc.BIG_W, dc.BIG_H, 2051) and not dc.window_fits(dc.BIG_W, dc.BIG_H, 2052)
    assert not dc.window_fits(dc.BIG_W, dc.BIG_H, dc.BIG_W)                  # at_window_ratio = 1: the whole image
    assert dc.window_fits(4096, 4096, 4096)                                   # 16.7 MP of 255 still fit
    assert all(dc.window_fits(w, h, w) for w, h in dc.SIZES)


def _candidates(img, p):
    fg = vco_detect.adaptive_threshold(img, p["at_threshold"], p["at_window_ratio"])
    boxes, area = dc.components(fg, img.shape[1], img.shape[0])
    ok = dc.passing(boxes, area, p["min_area"], p["min_density"], p["min_aspect"])
    return boxes[ok], area[ok]


def test_the_lattice_has_exactly_4096_candidates_and_its_variant_one_more():
    p = dc.params()
    img = dc.lattice_image()
    assert img.shape == (328, 328)
    boxes, area = _candidates(img, p)
    assert len(boxes) == 4096 and (area == 4).all()
    np.testing.assert_array_equal(0.5 * (boxes[:, :2] + boxes[:, 2:]), dc.lattice_centres())      # row-major, the closed form
    assert len(_candidates(dc.lattice_image(extra=True), p)[0]) == 4097
    # the restatement confirms the closed form of the centres on a small lattice
    cen, _, _ = dc.reference(dc.lattice_image(6, 5), p)
    np.testing.assert_allclose(cen, dc.lattice_centres(6, 5), rtol=0, atol=1e-9)


def test_the_faint_blob_is_a_candidate_without_a_gradient():
    img = dc.faint_image()
    boxes, area = _candidates(img, dc.FAINT_PARAMS)
    assert len(boxes) == 1 and area[0] == 16
    M, used = dc.normal_matrix(img, boxes[0])
    assert used == 0 and not M.any()
    cen, con, bx = dc.reference(img, dc.FAINT_PARAMS)
    assert cen.shape == (0, 2) and con.shape == (0, 3, 3) and bx.shape == (0, 4)
    assert len(_candidates(img, dc.params())[0]) == 0                          # at the defaults there is nothing at all


@pytest.mark.parametrize("w,h,n", [(72, 40, 1122), (100, 100, 4418)])
def test_the_checkerboard_is_all_candidates_and_no_gradient(w, h, n):
    """72 x 40: more candidates than travel in the first copy, every one without a gradient.  100 x 100: more than the device's limit."""
    img = dc.checker_image(w, h)
    boxes, area = _candidates(img, dc.CHECKER_PARAMS)
    assert len(boxes) == n and (area == 1).all()
    assert (n > 4096) == (w == 100) and n > 512
    gx, gy = vco_detect.gradient(img)
    assert not gx[:, 1:-1].any() and not gy[1:-1, :].any()
    if n <= 4096:
        assert all(dc.normal_matrix(img, b)[1] == 0 for b in boxes[::37])
        assert len(dc.reference(img, dc.CHECKER_PARAMS)[0]) == 0
