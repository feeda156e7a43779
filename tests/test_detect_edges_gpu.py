"""The dot detector (vc_detect.hip, eight kernels behind vc_detector_*) at its size, parameter and labelling edges, against the numpy
restatement (oracle/vco_detect.py) at the same parameters and against a second, independent labelling (scipy.ndimage).  The inputs and
what makes each of them a test are in detect_cases.py; test_detect_cases_cpu.py holds their conditions on the reference alone, and
every test here asserts the condition it stands on again before it looks at the device.

Bounds: centres 1e-7 px, conics 1e-9 on unit-norm matrices (the project's, tests/test_detect.py); boxes, counts and order exact.

Two rules of the C ABI are pinned here (include/vicalib_amd.h):
  * a threshold window whose largest possible sum does not fit 32 bits is refused (the integral image is kept modulo 2^32);
  * a candidate whose conic fit is singular is not a dot.  Tested for the case that has a definite answer on both sides: no pixel of
    the box reaches the gradient threshold, the matrix is zero.  Fits that are rank-deficient with a non-zero matrix (a single pixel,
    a straight run one pixel wide) stay out of scope: the restatement raises on them, and the inputs here hold none (checked).

Measured on the MI355X (every test prints its own figures): largest centre deviation 4.6e-13 px (the 19 MP image), largest
conic deviation 4.1e-14 (at_threshold = 0.12); most cases agree in the centres to the last bit.

What fails here under a wrong kernel (one edit of vc_detect.hip at a time, values only, tests/test_detect.py run beside it):
  * rad fixed at w / 30: the sizes 8 x 8, 9 x 33 and 15 x 40, the at_window_ratio cases, all six at once, the wrap -- test_detect.py
    stays green;
  * the carry of k_det_rows not added: 513, 1024 and 1025 columns (512 passes: one round), most parameter cases, the wrap; test_detect.py
    catches the lost carry too, at its two rounds -- new here are the one-pixel last round and the third round;
  * the density comparison of k_det_select reversed, or atomicMin on a piece's x0 replaced by a store: nearly everything in both files."""
import numpy as np
import pytest

import detect_cases as dc
from detect_cases import dot_images, vco_detect
from vicalib_amd.lib import ConicDetector, VicalibError

pytestmark = pytest.mark.gpu


def _detector(img, p):
    det = ConicDetector(img.shape[1], img.shape[0])
    det.set_params(**dc.device_params(p))
    return det


def _compare(tag, got, ref):
    """Device (centres, conics, boxes) against the restatement's: prints the largest deviations, then asserts the bounds."""
    (g_cen, g_con, g_box), (cen, con, box) = got, ref
    assert g_cen.shape == cen.shape, (tag, len(g_cen), len(cen))
    np.testing.assert_array_equal(g_box, box)
    dev_c = float(np.abs(g_cen - cen).max()) if len(cen) else 0.0
    dev_q = float(np.abs(g_con - con).max()) if len(cen) else 0.0
    print("detect-edges %s: %d dots, centre deviation %.3g px, conic deviation %.3g" % (tag, len(cen), dev_c, dev_q))
    assert dev_c <= dc.CENTRE_TOL and dev_q <= dc.CONIC_TOL, (tag, dev_c, dev_q)


# ---- sizes -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w,h", dc.SIZES)
def test_sizes_from_one_tile_down_and_across_the_row_rounds(w, h):
    """One, two and three rounds of k_det_rows (w <= 512, <= 1024, 1025), heights at which most wavefronts of k_det_cols get no row, images
    smaller than one labelling tile, down to the 8 x 8 that vc_detector_create accepts."""
    img, p, at = dc.size_case(w, h)
    assert int(w / p["at_window_ratio"]) >= 2
    ref = dc.reference(img, p)
    assert len(ref[0]) == len(at) >= 1                    # every blob drawn is a dot of the reference
    _compare("size %dx%d" % (w, h), _detector(img, p).find_conics(img), ref)


# ---- parameters ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(dc.PARAM_CASES))
def test_every_parameter_reaches_the_kernels(name):
    """Each of at_threshold, at_window_ratio, conic_min_area, conic_min_density and conic_min_aspect, in both directions, and all six at
    once on the inverted image: values at which the restatement finds other dots than at the defaults."""
    img = dc.param_image(name)
    p = dc.params(**dc.PARAM_CASES[name])
    ref, ref0 = dc.param_reference(name), dc.param_reference(None)
    assert ref[2].shape != ref0[2].shape or not np.array_equal(ref[2], ref0[2])
    det = _detector(img, p)
    _compare("parameters %s" % name, det.find_conics(img), ref)
    if name == "all_six_inverted":                        # back to the defaults on the same handle: nothing of the six is left behind
        det.set_params()
        _compare("parameters defaults after %s" % name, det.find_conics(dc.param_image()), ref0)


# ---- labelling -------------------------------------------------------------------------------------------------------------------
def _stress(name):
    mask = dc.stress_mask(name)
    h, w = mask.shape
    img = dc.mask_image(mask)
    p = dc.STRESS_PARAMS
    np.testing.assert_array_equal(vco_detect.adaptive_threshold(img, p["at_threshold"], p["at_window_ratio"]), mask)
    boxes, area = dc.components(mask, w, h)
    return img, boxes, area


def _check_labelling(tag, det, img, boxes):
    _, _, g_box = det.find_conics(img)
    print("detect-edges %s: %d components" % (tag, len(boxes)))
    assert len(g_box) == len(boxes), (tag, len(g_box), len(boxes))
    np.testing.assert_array_equal(g_box, boxes)           # same components, same boxes, same order


@pytest.mark.parametrize("name", ["spiral", "serpentine"])
def test_long_chains_in_the_union_find(name):
    """One component thousands of pixels long through nine tiles (spiral) and the longest chain one tile's LDS union-find can hold
    (serpentine), held to scipy's labelling."""
    img, boxes, area = _stress(name)
    assert len(boxes) == 1 and area[0] == (img == dc.DARK).sum() >= 500
    _check_labelling("labelling %s" % name, _detector(img, dc.STRESS_PARAMS), img, boxes)


def test_noise_components_against_an_independent_labelling():
    """Thresholded low-pass noise at two ragged sizes: hundreds of irregular components, many across tile edges.  The same image twice on
    one handle, with a handle of another size at work in between: no state is left behind or shared."""
    img_a, boxes_a, area_a = _stress("noise_97x71")
    img_b, boxes_b, area_b = _stress("noise_160x130")
    assert len(boxes_a) >= 100 and len(boxes_b) >= 300 and max(area_a.max(), area_b.max()) >= 100
    det_a, det_b = _detector(img_a, dc.STRESS_PARAMS), _detector(img_b, dc.STRESS_PARAMS)
    _check_labelling("labelling noise 97x71", det_a, img_a, boxes_a)
    _check_labelling("labelling noise 160x130", det_b, img_b, boxes_b)
    _check_labelling("labelling noise 97x71 again", det_a, img_a, boxes_a)
    _check_labelling("labelling noise 160x130 again", det_b, img_b, boxes_b)


# ---- candidate limit -------------------------------------------------------------------------------------------------------------
def test_exactly_4096_candidates_and_one_more():
    """64 x 64 blobs: the limit itself comes back whole (second download, ranking across all 16 workgroups of k_det_order), row-major, at
    the closed-form centres; one blob more is VC_ERR_UNSUPPORTED; the handle then works as a fresh one does."""
    p = dc.params()
    img, more = dc.lattice_image(), dc.lattice_image(extra=True)
    want = dc.lattice_centres()
    for im, n in ((img, 4096), (more, 4097)):
        fg = vco_detect.adaptive_threshold(im, p["at_threshold"], p["at_window_ratio"])
        boxes, area = dc.components(fg, im.shape[1], im.shape[0])
        assert dc.passing(boxes, area, p["min_area"], p["min_density"], p["min_aspect"]).sum() == n
    det = _detector(img, p)
    cen, con, box = det.find_conics(img)
    assert len(cen) == 4096
    np.testing.assert_array_equal(box, np.concatenate([want - 0.5, want + 0.5], axis=1).astype(np.int32))
    dev = float(np.abs(cen - want).max())
    print("detect-edges lattice: 4096 dots, centre deviation from the closed form %.3g px" % dev)
    assert dev <= dc.CENTRE_TOL
    assert con.shape == (4096, 3, 3) and np.abs(np.linalg.norm(con, axis=(1, 2)) - 1.0).max() < 1e-12
    with pytest.raises(VicalibError, match="VC_ERR_UNSUPPORTED"):
        det.find_conics(more)
    view, _ = dot_images.render(width=img.shape[1], height=img.shape[0], seed=4)
    after, fresh = det.find_conics(view), _detector(view, p).find_conics(view)
    assert len(fresh[0]) >= 20
    for a, b in zip(after, fresh):
        np.testing.assert_array_equal(a, b)
    _compare("view after the limit", after, dc.reference(view, p))


# ---- the 2^32 wrap and the window rule -------------------------------------------------------------------------------------------
def test_running_sums_wrap_and_a_window_that_cannot_fit_is_refused():
    """19 MP of 255: the 32-bit running sums pass 2^32 in the middle of a patch of dots and the four-corner differences still give every
    window's sum -- the device on the large image equals the restatement on the bottom-right crop (same half-width, every dot further
    than a window from the crop's cut edges).  On the same handle at_window_ratio = 1 makes the window the whole image, whose sum does
    not fit: refused, as is the first half-width at which the rule bites; the last one below it is accepted."""
    img = dc.big_image()
    crop, (ox, oy) = dc.big_crop()
    rad = dc.BIG_RAD
    r_big, r_crop = dc.ratio_for(dc.BIG_W, rad), dc.ratio_for(dc.BIG_CROP, rad)
    assert int(dc.BIG_W / r_big) == int(dc.BIG_CROP / r_crop) == rad
    assert int(img[:dc.BIG_Y, :dc.BIG_X].sum(dtype=np.int64)) < 2 ** 32 < int(img[:dc.BIG_Y + dc.BIG_PATCH, :dc.BIG_X + dc.BIG_PATCH].sum(dtype=np.int64))
    cen, con, box = dc.reference(crop, dc.params(at_window_ratio=r_crop))
    assert len(cen) >= 20 and box[:, 0].min() > 2 * rad + 1 + 2 and box[:, 1].min() > 2 * rad + 1 + 2
    det = ConicDetector(dc.BIG_W, dc.BIG_H)
    try:
        for ratio in (1.0, dc.ratio_for(dc.BIG_W, 2052)):
            assert not dc.window_fits(dc.BIG_W, dc.BIG_H, int(dc.BIG_W / ratio))
            det.set_params(at_window_ratio=ratio)
            with pytest.raises(VicalibError, match="VC_ERR_UNSUPPORTED"):
                det.find(img)
        det.set_params(**dc.device_params(dc.params(at_window_ratio=r_big)))
        g_cen, g_con, g_box = det.find_conics(img)
        assert g_cen.shape == cen.shape
        np.testing.assert_array_equal(g_box - np.array([ox, oy, ox, oy]), box)
        dev = float(np.abs(g_cen - np.array([ox, oy]) - cen).max())
        print("detect-edges wrap: %d dots, centre deviation %.3g px" % (len(cen), dev))
        assert dev <= dc.CENTRE_TOL
        assert dc.window_fits(dc.BIG_W, dc.BIG_H, 2051)
        det.set_params(at_window_ratio=dc.ratio_for(dc.BIG_W, 2051))      # the largest window the rule lets through: its sum fits, the
        assert len(det.find(img)) == len(cen)                              # local mean is near 255 everywhere, the same dots are dots
    finally:
        det.close()


# ---- degenerate fits -------------------------------------------------------------------------------------------------------------
def test_a_component_without_a_gradient_is_not_a_dot():
    """A 4 x 4 blob of 224 on 225 at at_threshold = 0.999 is a candidate whose fit has nothing to fit (matrix zero): no dot on either
    side, and the ordinary image that follows on the same handle comes out as on a fresh one."""
    img = dc.faint_image()
    p = dc.FAINT_PARAMS
    fg = vco_detect.adaptive_threshold(img, p["at_threshold"], p["at_window_ratio"])
    boxes, area = dc.components(fg, img.shape[1], img.shape[0])
    assert len(boxes) == 1 and dc.passing(boxes, area, p["min_area"], p["min_density"], p["min_aspect"]).all()
    assert dc.normal_matrix(img, boxes[0])[1] == 0 and len(dc.reference(img, p)[0]) == 0
    det = _detector(img, p)
    cen, con, box = det.find_conics(img)
    assert cen.shape == (0, 2) and con.shape == (0, 3, 3) and box.shape == (0, 4)
    assert det.find(img).shape == (0, 2)
    view, _ = dot_images.render(seed=1)
    _compare("view after the faint blob", det.find_conics(view), dc.reference(view, p))
    det.set_params()
    _compare("view after the faint blob, defaults", det.find_conics(view), dc.reference(view, dc.params()))


def test_a_checkerboard_holds_no_dot_and_the_limit_counts_candidates():
    """Every dark pixel of a checkerboard is a candidate (min_area = 1) and none has a gradient: 1122 candidates, more than travel in
    the first copy, no dot.  The limit of 4096 stays on the candidates: 4418 of them are refused although none would be a dot."""
    p = dc.CHECKER_PARAMS
    img = dc.checker_image(72, 40)
    boxes, _ = dc.components(vco_detect.adaptive_threshold(img, p["at_threshold"], p["at_window_ratio"]), 72, 40)
    assert len(boxes) == 1122 and len(dc.reference(img, p)[0]) == 0
    det = _detector(img, p)
    assert det.find_conics(img)[0].shape == (0, 2)
    big = dc.checker_image(100, 100)
    assert len(dc.components(vco_detect.adaptive_threshold(big, p["at_threshold"], p["at_window_ratio"]), 100, 100)[0]) == 4418
    with pytest.raises(VicalibError, match="VC_ERR_UNSUPPORTED"):
        _detector(big, p).find(big)
