"""TEST INFRASTRUCTURE: the inputs of the dot detector's edge tests and the reference helpers they share.  No GPU in here.

tests/test_detect_cases_cpu.py checks on the numpy restatement (oracle/vco_detect.py) alone that every input does what it is meant to do
(a parameter case changes the result, the large image wraps a 32-bit sum, the lattice has exactly 4096 candidates, ...);
tests/test_detect_edges_gpu.py runs the same inputs through the HIP kernels (vc_detect.hip).  Everything is deterministic and seeded.

Geometry the builders rely on (vc_detect.hip): k_det_rows walks a row in rounds of 512 pixels with a carry; k_det_cols gives each of 16
wavefronts (h + 15) / 16 rows; labelling tiles are 32 x 32; the count and the first 512 records come back in one copy; at most 4096
candidates per image.  A candidate's box must keep 3 pixels to every image edge (the border rule of find_conics)."""
import functools
import os
import sys

import numpy as np
from scipy import ndimage

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "oracle"))
import dot_images          # noqa: E402
import vco_detect          # noqa: E402

WHITE, DARK = 225, 30
DEFAULTS = dict(at_threshold=0.9, at_window_ratio=30.0, min_area=4.0, min_density=0.6, min_aspect=0.2)
CENTRE_TOL, CONIC_TOL = 1e-7, 1e-9          # the project's bounds (tests/test_detect.py)


def params(**kw):
    """Restatement keywords: the defaults with `kw` on top."""
    bad = set(kw) - set(DEFAULTS) - {"black_on_white"}
    assert not bad, bad
    return dict(DEFAULTS, **kw)


def device_params(p):
    """The same values under the names ConicDetector.set_params takes."""
    return dict(black_on_white=p.get("black_on_white", True), at_threshold=p["at_threshold"], at_window_ratio=p["at_window_ratio"],
                conic_min_area=p["min_area"], conic_min_density=p["min_density"], conic_min_aspect=p["min_aspect"])


def ratio_for(w, rad):
    """An at_window_ratio that gives exactly the half-width `rad` at width w on both sides (rad = int(w / ratio))."""
    r = w / (rad + 0.5)
    assert int(w / r) == rad
    return r


def reference(img, p):
    return vco_detect.find_conics(img, full=True, **p)


# ---- the second labelling reference --------------------------------------------------------------------------------------------
def components(fg, w, h):
    """4-connected components of the mask `fg` by scipy.ndimage (shares nothing with vco_detect.label4): boxes [n, 4] (x0, y0, x1, y1
    inclusive) and areas [n] of the components that pass the border rule of find_conics, ordered by their smallest pixel index."""
    fg = np.asarray(fg, dtype=bool)
    assert fg.shape == (h, w)
    lab, n = ndimage.label(fg, structure=[[0, 1, 0], [1, 1, 1], [0, 1, 0]])
    if n == 0:
        return np.zeros((0, 4), dtype=np.int64), np.zeros(0, dtype=np.int64)
    idx = np.arange(1, n + 1)
    first = np.asarray(ndimage.minimum(np.arange(h * w, dtype=np.int64).reshape(h, w), lab, idx), dtype=np.int64)
    area = np.bincount(lab.ravel(), minlength=n + 1)[1:].astype(np.int64)
    boxes = np.array([(s[1].start, s[0].start, s[1].stop - 1, s[0].stop - 1) for s in ndimage.find_objects(lab)], dtype=np.int64)
    x0, y0, x1, y1 = boxes.T
    keep = (x0 - 2 >= 1) & (y0 - 2 >= 1) & (x1 + 1 + 2 <= w - 1) & (y1 + 1 + 2 <= h - 1)
    order = np.argsort(first[keep], kind="stable")
    return boxes[keep][order], area[keep][order]


def passing(boxes, area, min_area, min_density, min_aspect):
    """Which of these components pass the area, density and aspect tests of find_conics."""
    bw, bh = boxes[:, 2] - boxes[:, 0] + 1, boxes[:, 3] - boxes[:, 1] + 1
    return (area >= min_area) & (area >= min_density * bw * bh) & (np.minimum(bw, bh) >= min_aspect * np.maximum(bw, bh))


def normal_matrix(img, box):
    """The 5 x 5 matrix of fit_dual_conic for a component's box (inclusive, not yet grown) and the number of pixels that enter it."""
    gx, gy = vco_detect.gradient(img)
    x0, y0, x1, y1 = box[0] - vco_detect.GROW, box[1] - vco_detect.GROW, box[2] + 1 + vco_detect.GROW, box[3] + 1 + vco_detect.GROW
    cx, cy = 0.5 * (x0 + x1 - 1), 0.5 * (y0 + y1 - 1)
    y, x = np.mgrid[y0:y1, x0:x1]
    a, b = gx[y0:y1, x0:x1], gy[y0:y1, x0:x1]
    w2 = a * a + b * b
    use = w2 >= vco_detect.MIN_GRAD2
    c = -(a * (x - cx) + b * (y - cy))
    K = np.stack([a * a, a * b, b * b, a * c, b * c], axis=-1)[use]
    return np.einsum("n,ni,nj->ij", w2[use], K, K), int(use.sum())


def mask_image(mask):
    return np.where(mask, DARK, WHITE).astype(np.uint8)


def disc(img, cx, cy, r, value, r_in=0.0, ax=1.0, ay=1.0):
    """Hard-edged ellipse (semi-axes r * ax, r * ay), optionally a ring down to the relative radius r_in / r."""
    yy, xx = np.mgrid[0:img.shape[0], 0:img.shape[1]]
    q = ((xx - cx) / (r * ax)) ** 2 + ((yy - cy) / (r * ay)) ** 2
    img[(q < 1.0) & (q >= (r_in / r) ** 2)] = value


# ---- sizes -----------------------------------------------------------------------------------------------------------------------
SIZES = [(8, 8), (9, 33), (33, 9), (15, 40), (31, 31), (32, 32), (33, 33), (512, 40), (513, 40), (1024, 24), (1025, 24)]      # w x h


def _spread(cands, limit):
    """Blob origins from `cands` that keep the border rule (origin >= 3, origin + 1 <= limit - 4) and 4 pixels between each other."""
    out = []
    for c in sorted(set(cands)):
        if 3 <= c and c + 1 <= limit - 4 and all(abs(c - o) >= 4 for o in out):
            out.append(c)
    return out


def size_case(w, h):
    """2 x 2 dark blobs on 225 wherever they fit: in the corners that the border rule leaves, in the middle, on both sides of the 512-pixel
    rounds of k_det_rows (x = 509..510 and 513..514; 1021..1022 would need w >= 1026 and fits none of SIZES) and at the last columns that
    pass the border rule (w - 5, w - 4).  From 512 columns on the half-width is 4, so the window of the last blob reaches the last
    entry of the integral image's row, the one the last round of k_det_rows writes with the carry of all rounds before it.
    -> (image, parameters, blob origins [(x, y)])."""
    rad = 4 if w >= 512 else 2
    xs = _spread([3, w - 5, 509, 513, 1021, w // 2 - 1, 250, 760], w)
    ys = _spread([3, h - 5, h // 2 - 1], h)
    img = np.full((h, w), WHITE, dtype=np.uint8)
    at = [(x, y) for y in ys for x in xs]
    for x, y in at:
        img[y:y + 2, x:x + 2] = DARK
    return img, params(at_window_ratio=ratio_for(w, rad)), at


# ---- parameters ------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _param_image():
    img, _ = dot_images.render()                         # 640 x 480, 54 dots of 25 on 230 in the middle
    img[200:203, 10:300] = 20                            # a 3-px line through the dots' rows: fails the aspect test
    img[400:402, 500:502] = 20                           # 4 pixels: just passes min_area = 4
    img[60:66, 60:66] = 20; img[62:64, 62:64] = 230      # 6 x 6 with a 2 x 2 hole: density 32 / 36
    img[60:64, 120:140] = 20                             # 4 x 20 bar: aspect exactly 0.2
    disc(img, 320.0, 60.0, 22.0, 20, ax=1.0, ay=0.12)    # thin ellipse 43 x 5: aspect below 0.2, a dot once min_aspect is loosened
    disc(img, 560.0, 80.0, 10.3, 20, r_in=7.2)           # ring: density below 0.6, a dot once min_density is loosened
    disc(img, 80.0, 420.0, 7.3, 212)                     # faint disc, 212 on 230: a dot only above at_threshold = 0.93
    disc(img, 585.0, 425.0, 40.3, 150)                   # mid-grey plateau with a dot on it: found against the plateau by a small
    disc(img, 585.0, 425.0, 6.3, 40)                     # window, swallowed by the plateau under a large one
    img.setflags(write=False)
    return img


PARAM_CASES = {
    "min_area_5": dict(min_area=5.0),
    "min_aspect_0.21": dict(min_aspect=0.21),
    "min_aspect_0.1": dict(min_aspect=0.1),
    "min_density_0.9": dict(min_density=0.9),
    "min_density_0.3": dict(min_density=0.3),
    "at_threshold_0.12": dict(at_threshold=0.12),
    "at_threshold_0.95": dict(at_threshold=0.95),
    "at_window_ratio_640": dict(at_window_ratio=640.0),
    "at_window_ratio_1000": dict(at_window_ratio=1000.0),
    "at_window_ratio_4": dict(at_window_ratio=4.0),
    "all_six_inverted": dict(black_on_white=False, at_threshold=0.85, at_window_ratio=20.0, min_area=6.0, min_density=0.5, min_aspect=0.3),
}


def param_image(name=None):
    """The image of the parameter cases; for a case with black_on_white = False its inverse (white dots on black)."""
    img = _param_image()
    if name is not None and PARAM_CASES[name].get("black_on_white", True) is False:
        return 255 - img
    return img


@functools.lru_cache(maxsize=None)
def param_reference(name=None):
    """(centres, conics, boxes) of the restatement for a parameter case; None: the defaults."""
    return reference(param_image(name), params(**(PARAM_CASES[name] if name else {})))


# ---- labelling stress ------------------------------------------------------------------------------------------------------------
STRESS_PARAMS = params(min_area=1.0, min_density=0.0, min_aspect=0.0, at_window_ratio=2.0)      # (a window of half the width: the local mean of a
#                                                                                                  whole neighbourhood, so that image and mask agree)


def spiral_mask(size=110, n=96):
    """A one-pixel square spiral with one-pixel gaps filling n x n in the middle of size x size: ONE component, thousands of pixels long,
    through nine tiles."""
    m = np.zeros((size, size), dtype=bool)
    x = y = (size - n) // 2
    m[y, x] = True
    # sides: n-1 right, n-1 down, n-1 left, then n-3 up, n-3 right, n-5 down, n-5 left, ...
    lengths = [n - 1, n - 1, n - 1] + [v for k in range(n - 3, 0, -2) for v in (k, k)]
    dirs = ((1, 0), (0, 1), (-1, 0), (0, -1))
    for i, ln in enumerate(lengths):
        dx, dy = dirs[i % 4]
        for _ in range(ln):
            x += dx; y += dy
            m[y, x] = True
    return m


def serpentine_mask(size=100, t=32):
    """A one-pixel serpentine confined to the tile [32, 64) x [32, 64): every second row, joined at alternating ends."""
    m = np.zeros((size, size), dtype=bool)
    for k, y in enumerate(range(t, 2 * t, 2)):
        m[y, t:2 * t] = True
        if y + 2 < 2 * t:
            m[y + 1, 2 * t - 1 if k % 2 == 0 else t] = True
    return m


def noise_mask(w, h, seed):
    """Thresholded low-pass noise: a few hundred irregular components, many of them across tile edges.  Components that are one pixel
    wide or high from end to end (single pixels, straight runs) are cleared: the normal equations of their conic fit are singular, and
    what happens to such a candidate is not what these images test."""
    rng = np.random.default_rng(seed)
    f = ndimage.gaussian_filter(rng.standard_normal((h, w)), 0.7)
    m = f > np.quantile(f, 0.7)
    lab, n = ndimage.label(m, structure=[[0, 1, 0], [1, 1, 1], [0, 1, 0]])
    for k, s in enumerate(ndimage.find_objects(lab)):
        if s[0].stop - s[0].start == 1 or s[1].stop - s[1].start == 1:
            m[s][lab[s] == k + 1] = False
    return m


STRESS = {
    "spiral": lambda: spiral_mask(),
    "serpentine": lambda: serpentine_mask(),
    "noise_97x71": lambda: noise_mask(97, 71, 11),
    "noise_160x130": lambda: noise_mask(160, 130, 12),
}


@functools.lru_cache(maxsize=None)
def stress_mask(name):
    m = STRESS[name]()
    m.setflags(write=False)
    return m


# ---- candidate limit -------------------------------------------------------------------------------------------------------------
def lattice_image(nx=64, ny=64, pitch=5, extra=False):
    """nx x ny blobs of 2 x 2 at x = 4 + pitch i, y = 4 + pitch j (centres 4.5 + pitch i, 4.5 + pitch j) with 7 pixels of margin at the far
    edges; extra: one more blob in that margin, right of the first row."""
    w, h = 4 + pitch * nx + 4, 4 + pitch * ny + 4
    img = np.full((h, w), WHITE, dtype=np.uint8)
    for j in range(ny):
        for i in range(nx):
            img[4 + pitch * j:6 + pitch * j, 4 + pitch * i:6 + pitch * i] = DARK
    if extra:
        img[4:6, w - 5:w - 3] = DARK
    return img


def lattice_centres(nx=64, ny=64, pitch=5):
    j, i = np.mgrid[0:ny, 0:nx]
    return np.stack([4.5 + pitch * i.ravel(), 4.5 + pitch * j.ravel()], axis=1)


# ---- degenerate fits -------------------------------------------------------------------------------------------------------------
FAINT_PARAMS = params(at_threshold=0.999)


def faint_image(w=640, h=480):
    """A 4 x 4 blob of 224 on 225: a component at at_threshold = 0.999 whose gradients (0.5 grey levels per pixel) all stay below
    MIN_GRAD2, so that the fit's matrix is zero."""
    img = np.full((h, w), 225, dtype=np.uint8)
    img[200:204, 300:304] = 224
    return img


CHECKER_PARAMS = params(min_area=1.0, min_density=0.0, min_aspect=0.0)


def checker_image(w, h):
    """A checkerboard over the whole image: every dark pixel is a component of its own, and every central difference an image holds
    away from its border vanishes."""
    yy, xx = np.mgrid[0:h, 0:w]
    return mask_image((xx + yy) % 2 == 0)


# ---- the 2^32 wrap ---------------------------------------------------------------------------------------------------------------
BIG_W, BIG_H, BIG_PATCH, BIG_X, BIG_Y, BIG_CROP, BIG_RAD = 4608, 4126, 300, 4202, 3720, 512, 8


@functools.lru_cache(maxsize=None)
def big_patch():
    img, _ = dot_images.render(width=BIG_PATCH, height=BIG_PATCH, white=255)
    return img


def big_image():
    """19 MP of 255 with a rendered 300 x 300 patch of dots at (4202, 3720), in the middle of the bottom-right 512 x 512: the exact integral
    image is below 2^32 at the patch's top-left corner, reaches it near the patch's centre (4352 * 3870 * 255 = 2^32 + 1.6e5) and is
    above it at its bottom-right corner, so the 32-bit running sums wrap INSIDE the patch, among the dots."""
    img = np.full((BIG_H, BIG_W), 255, dtype=np.uint8)
    img[BIG_Y:BIG_Y + BIG_PATCH, BIG_X:BIG_X + BIG_PATCH] = big_patch()
    return img


def big_crop():
    """The bottom-right 512 x 512 of big_image() and its offset (x, y) in it, built without the large image."""
    ox, oy = BIG_W - BIG_CROP, BIG_H - BIG_CROP
    img = np.full((BIG_CROP, BIG_CROP), 255, dtype=np.uint8)
    img[BIG_Y - oy:BIG_Y - oy + BIG_PATCH, BIG_X - ox:BIG_X - ox + BIG_PATCH] = big_patch()
    return img, (ox, oy)


def window_fits(w, h, rad):
    """The rule of vc_detector_find_conics: the largest sum a clamped window can hold fits 32 bits."""
    return min(2 * rad + 1, w) * min(2 * rad + 1, h) * 255 < 2 ** 32
