"""TEST INFRASTRUCTURE shared by test_undistort_cpu.py and test_undistort_gpu.py: the cases, the oracle's side of every comparison
(oracle_lib.project, computed once per case and kept), and the checks themselves -- written against plain arrays, so that the same
check holds the host build of the kernels' arithmetic (tests/host_harness/undistort_harness.cpp) and the GPU kernels."""
import functools
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import oracle_lib as ol          # noqa: E402
from vicalib_amd import synth    # noqa: E402

MODELS = ("fov", "poly2", "poly3", "kb4", "linear", "rational6")
SRC, DST = (53, 41), (67, 35)                     # no multiple of 4 or 64
FULL = (640, 480)                                 # the size the generator's ground-truth intrinsics belong to
BEYOND_K = np.array([400.0, 400.0, 320.0, 240.0, -0.6, 0.0, 0.0])      # poly3 whose profile r (1 - 0.6 r^2) has a maximum at r = 0.745


def gt(model):
    return np.array(synth.GT_INTRINSICS[synth.MODEL_IDS[model]], dtype=np.float64)


def rotation(deg):
    from scipy.spatial.transform import Rotation as R
    return R.from_euler("xyz", deg, degrees=True).as_matrix()


ROTATIONS = {"identity": np.eye(3), "rotated": rotation((4.0, -7.0, 3.0))}


def project(model, K, rays):
    """oracle_lib.project of every ray [n, 3] -> [n, 2]"""
    m = synth.MODEL_IDS[model]
    return np.array([ol.project(m, np.ascontiguousarray(r), K)[0] for r in np.asarray(rays, dtype=np.float64).reshape(-1, 3)])


def ray_at(model, t, phi):
    """the ray at radial coordinate t (tan of the angle off the axis; the angle itself for kb4) and azimuth phi"""
    t, phi = np.asarray(t, dtype=np.float64), np.asarray(phi, dtype=np.float64)
    if model == "kb4":
        return np.stack([np.sin(t) * np.cos(phi), np.sin(t) * np.sin(phi), np.cos(t)], axis=-1)
    return np.stack([t * np.cos(phi), t * np.sin(phi), np.ones_like(t)], axis=-1)


def profile(model, K, t):
    """the oracle's radial profile r_d(t) at unit focal length (fu = fv in every case here)"""
    pix = project(model, K, ray_at(model, t, np.zeros_like(t)))
    return (pix[:, 0] - K[2]) / K[0]


def t_of_radius(model, K, rd):
    """the smallest t with profile(t) = rd: first crossing on a grid of the oracle's profile, then bisection"""
    grid = np.arange(0.0, 1.55 if model == "kb4" else 4.0, 0.01)
    above = np.nonzero(profile(model, K, grid) >= rd)[0]
    assert len(above), (model, rd)
    if above[0] == 0:
        return 0.0
    lo, hi = grid[above[0] - 1], grid[above[0]]
    for _ in range(60):
        mid = 0.5 * (lo + hi)
        if profile(model, K, np.array([mid]))[0] < rd:
            lo = mid
        else:
            hi = mid
    return 0.5 * (lo + hi)


def unproject(model, K, px):
    """oracle-side inverse of one pixel (bisection): its ray"""
    d = (np.asarray(px, dtype=np.float64) - K[2:4]) / K[:2]
    return ray_at(model, t_of_radius(model, K, np.hypot(*d)), np.arctan2(d[1], d[0]))


@functools.lru_cache(maxsize=None)
def field_t_max(model, frac=0.95):
    """t of the rays that land at `frac` of the half-diagonal of the full-size image"""
    K = gt(model)
    return t_of_radius(model, K, frac * np.hypot(FULL[0] / 2.0, FULL[1] / 2.0) / K[0])


@functools.lru_cache(maxsize=None)
def profile_samples(model):
    """(t, r_d) of 512 radii over the field the tests sample (to 96 % of the half-diagonal), from the oracle"""
    t = np.linspace(0.0, field_t_max(model, 0.96), 512)
    return t, profile(model, gt(model), t)


def assert_profile_increasing(model, max_inverse_slope=10.0):
    """CPU precondition: over the sampled radii the oracle's profile is increasing -- every sampled pixel has one preimage -- and no
    flatter than 1 / max_inverse_slope"""
    t, rd = profile_samples(model)
    slope = np.diff(rd) / np.diff(t)
    assert np.all(slope > 0.0), (model, slope.min())
    assert np.all(1.0 / slope < max_inverse_slope), (model, (1.0 / slope).max())


# ------------------------------------------------------------------------------------------------------------ the map
@functools.lru_cache(maxsize=None)
def map_case(model, rot):
    """Source SRC with the model's ground-truth intrinsics -- a window at the top left corner of the model's field, where the distortion is
    strongest --, destination DST: a pinhole camera whose centre pixel looks (through R_ds) at the source window's centre pixel, with focal
    lengths that make the destination image about one and a half times the window's footprint, so that a good part of the entries has a
    source pixel and a good part has none.  Returns K, dst_linear, R_ds and the oracle's source coordinate of every destination pixel
    [h, w, 2] with its z in the source frame [h, w]."""
    K = gt(model)
    # kb4's window lies 82 degrees off the axis: turned by R_ds it falls behind the destination camera, so there the rotation is taken as
    # R_sd (the destination turned towards the window)
    R_ds = ROTATIONS[rot].T if model == "kb4" else ROTATIONS[rot]
    c = R_ds @ unproject(model, K, ((SRC[0] - 1) / 2.0, (SRC[1] - 1) / 2.0))
    assert c[2] > 0.1
    ci, cj = (DST[0] - 1) / 2.0, (DST[1] - 1) / 2.0

    def centred(fu, fv):
        return np.array([fu, fv, ci - fu * c[0] / c[2], cj - fv * c[1] / c[2]])

    def src_of(dl, i, j):
        return project(model, K, (R_ds.T @ np.array([(i - dl[2]) / dl[0], (j - dl[3]) / dl[1], 1.0]))[None])[0]

    d0 = centred(K[0], K[1])
    sx = np.linalg.norm(src_of(d0, ci + 1, cj) - src_of(d0, ci - 1, cj)) / 2          # source pixels per destination pixel at the centre
    sy = np.linalg.norm(src_of(d0, ci, cj + 1) - src_of(d0, ci, cj - 1)) / 2
    dl = centred(K[0] * sx / (0.65 * SRC[0] / ci), K[1] * sy / (0.65 * SRC[1] / cj))
    return (K, dl, R_ds) + oracle_map(model, K, dl, R_ds, SRC, DST)


@functools.lru_cache(maxsize=None)
def behind_case():
    """poly3, the destination camera turned by 100 degrees about y: part of its rays have z <= 0 in the source frame"""
    K = gt("poly3")
    R_ds = rotation((0.0, 100.0, 0.0))
    dl = np.array([40.0, 40.0, 33.0, 17.0])
    src = (FULL[0], FULL[1])
    return (K, dl, R_ds, src) + oracle_map("poly3", K, dl, R_ds, src, DST)


def oracle_map(model, K, dl, R_ds, src, dst):
    jj, ii = np.meshgrid(np.arange(dst[1]), np.arange(dst[0]), indexing="ij")
    rays_d = np.stack([(ii - dl[2]) / dl[0], (jj - dl[3]) / dl[1], np.ones(ii.shape)], axis=-1)
    rays_s = rays_d @ R_ds                                     # R_sd ray = R_ds^T ray, row vectors
    with np.errstate(all="ignore"):
        pix = project(model, K, rays_s).reshape(dst[1], dst[0], 2)
    return pix, rays_s[..., 2]


def check_map(model, src, got_map, got_valid, want_pix, z_s):
    """Valid entries agree with the oracle to the fp32 rounding of the stored map; the valid mask agrees wherever the oracle's
    coordinate is further than 1e-6 px from the border of [0, w - 1] x [0, h - 1]; every ray with z <= 0 is invalid (not kb4)."""
    got_map = np.asarray(got_map); got_valid = np.asarray(got_valid, dtype=bool)
    x, y = want_pix[..., 0], want_pix[..., 1]
    with np.errstate(invalid="ignore"):
        finite = np.isfinite(x) & np.isfinite(y)
        front = (z_s > 0.0) | (model == "kb4")
        # signed distance to the border of the valid rectangle, positive inside
        inside_by = np.minimum(np.minimum(x, src[0] - 1.0 - x), np.minimum(y, src[1] - 1.0 - y))
    want_valid = finite & front & (inside_by >= 0.0)
    decided = ~(finite & front) | (np.abs(inside_by) > 1e-6)
    assert np.array_equal(got_valid[decided], want_valid[decided]), (model, np.argwhere(decided & (got_valid != want_valid))[:5])
    assert not got_valid[~front].any()
    assert np.all(np.isnan(got_map[~got_valid])) and not np.isnan(got_map[got_valid]).any()
    both = got_valid & want_valid
    for k in range(2):
        w = want_pix[..., k][both]
        tol = np.spacing(np.abs(w).astype(np.float32)).astype(np.float64) / 2 + 1e-9
        err = np.abs(got_map[..., k][both].astype(np.float64) - w)
        assert np.all(err <= tol), (model, k, (err / tol).max())
    return int(want_valid.sum()), int((~want_valid).sum())


# ------------------------------------------------------------------------------------------------------------ the remap
def remap_reference(m, imgs, fill):
    """The bilinear rule evaluated in float64 from the stored map m [h, w, 2] (float32): (rounded uint8 [n, h, w], unrounded value,
    valid mask)."""
    imgs = np.asarray(imgs)
    n, hs, ws = imgs.shape
    valid = ~np.isnan(m[..., 0])
    x = np.where(valid, m[..., 0], 0).astype(np.float64); y = np.where(valid, m[..., 1], 0).astype(np.float64)
    x0 = np.minimum(np.floor(x), ws - 2).astype(int); y0 = np.minimum(np.floor(y), hs - 2).astype(int)
    ax, ay = x - x0, y - y0
    p = imgs.astype(np.float64)
    p00, p01, p10, p11 = p[:, y0, x0], p[:, y0, x0 + 1], p[:, y0 + 1, x0], p[:, y0 + 1, x0 + 1]
    v = (1 - ay) * ((1 - ax) * p00 + ax * p01) + ay * ((1 - ax) * p10 + ax * p11)
    out = np.floor(v + 0.5).astype(np.uint8)
    out[:, ~valid] = fill
    return out, v, valid


def check_remap(got, m, imgs, fill):
    """Equal everywhere, except that one grey level is allowed exactly where the unrounded value lies within 1e-6 of a half-integer;
    returns the number of such pixels that differ."""
    want, v, valid = remap_reference(m, imgs, fill)
    got = np.asarray(got)
    assert np.all(got[:, ~valid] == fill)
    near_half = np.abs((v + 0.5) - np.rint(v + 0.5)) < 1e-6
    diff = got.astype(int) - want.astype(int)
    assert np.all(diff[~near_half | ~valid[None]] == 0), np.argwhere(diff != 0)[:5]
    assert np.all(np.abs(diff) <= 1)
    return int(np.count_nonzero(diff))


# ------------------------------------------------------------------------------------------------------------ points
@functools.lru_cache(maxsize=None)
def point_case(model, n=4096):
    """n rays spread over the model's field to 95 % of the full-size image's half-diagonal (uniform in t^2 and azimuth), through the
    oracle into source pixels; the destination is a pinhole camera rotated by R_ds.  Returns K, dst_linear, R_ds, the source pixels
    and the linear projection of the same rays (what vc_undistort_points must return).  kb4's field reaches 84 degrees off the axis:
    its destination is not rotated, since a pinhole camera turned by 7 degrees has no image of rays beyond 90 degrees in its own frame
    and magnifies any error by 1 + r_u^2 on the way there, which the 1e-8 px of the round trip has no room for."""
    rot = "identity" if model == "kb4" else "rotated"
    K = gt(model)
    rng = np.random.default_rng(11 + synth.MODEL_IDS[model])
    t = field_t_max(model) * np.sqrt(rng.uniform(0.0, 1.0, n)); phi = rng.uniform(-np.pi, np.pi, n)
    rays = ray_at(model, t, phi)
    R_ds = ROTATIONS[rot]
    dl = np.array([310.0, 295.0, 301.5, 255.25])
    return (K, dl, R_ds, project(model, K, rays)) + (linear_projection(rays, R_ds, dl),)


@functools.lru_cache(maxsize=None)
def kb4_rotated_point_case(n=1024):
    """kb4 rays to 60 degrees off the axis through the rotation of (4, -7, 3) degrees: point_case leaves kb4 unrotated"""
    K = gt("kb4")
    rng = np.random.default_rng(23)
    rays = ray_at("kb4", np.radians(60.0) * np.sqrt(rng.uniform(0.0, 1.0, n)), rng.uniform(-np.pi, np.pi, n))
    R_ds = ROTATIONS["rotated"]
    dl = np.array([310.0, 295.0, 301.5, 255.25])
    return (K, dl, R_ds, project("kb4", K, rays)) + (linear_projection(rays, R_ds, dl),)


def linear_projection(rays_s, R_ds, dl):
    """(pixels in the destination camera, z > 0 there)"""
    r = rays_s @ R_ds.T
    with np.errstate(all="ignore"):
        return np.stack([dl[0] * r[:, 0] / r[:, 2] + dl[2], dl[1] * r[:, 1] / r[:, 2] + dl[3]], axis=-1), r[:, 2] > 0


@functools.lru_cache(maxsize=None)
def line_case(model):
    """points of three 3-D straight lines in front of the source camera, inside the model's field: their source pixels (oracle)"""
    K = gt(model)
    s = np.linspace(-1.0, 1.0, 48)[:, None]
    lines = [np.array([0.05, -0.3, 1.0]) + s * np.array([0.45, 0.1, 0.2]),
             np.array([-0.2, 0.1, 1.2]) + s * np.array([0.1, 0.5, -0.15]),
             np.array([0.1, 0.25, 0.8]) + s * np.array([-0.4, 0.3, 0.1])]
    return K, [project(model, K, L) for L in lines]


def max_off_line(p):
    """largest distance of the points [n, 2] from their total-least-squares line"""
    q = p - p.mean(axis=0)
    return float(np.abs(q @ np.linalg.svd(q, full_matrices=False)[2][1]).max())


def border_samples(size, per_edge=97):
    w, h = size
    s = np.linspace(0.0, 1.0, per_edge)
    return np.concatenate([np.stack([s * (w - 1), 0 * s], 1), np.stack([s * (w - 1), 0 * s + h - 1], 1), np.stack([0 * s, s * (h - 1)], 1),
                           np.stack([0 * s + w - 1, s * (h - 1)], 1)])
