"""The held-out problems of the hold-out tests, built once and shared: the CPU test checks that the host reference (holdout_ref)
converges on every non-degenerate frame of every case from the very seeds the GPU tests use, the GPU tests compare against it.
A case is a dict: models, cams [(model id, K, T_ck)] (ground truth), grid_points, tiles [(held-out frame, camera, dot ids, pix)],
n_frames, seeds [n_frames, 7], fitted (held-out frames that have >= 4 corners)."""
import functools

import numpy as np

import holdout_ref as hr
from vicalib_amd import synth

ALL_MODELS = ["fov", "poly2", "poly3", "kb4", "linear", "rational6"]


def perturbed(T, key, dt=0.01, dr=np.deg2rad(1.0)):
    """T * exp([v, w]) with |v| = dt, |w| = dr in directions drawn from `key`."""
    rng = np.random.default_rng(1000 + key)
    v = rng.normal(size=3); w = rng.normal(size=3)
    return hr.se3_exp_apply(T, np.concatenate([dt * v / np.linalg.norm(v), dr * w / np.linalg.norm(w)]))


def _case(p, tiles, held, seeds):
    cams = [(p.cam_model[c], p.cam_K_gt[c], p.cam_T_ck_gt[c]) for c in range(len(p.cam_model))]
    n = len(held)
    count = np.zeros(n, dtype=int)
    for (f, c, ids, px) in tiles:
        count[f] += len(ids)
    return dict(p=p, cams=cams, grid_points=p.grid_points, tiles=tiles, n_frames=n, seeds=np.array(seeds), gt=p.frame_T_wk_gt[held],
                fitted=[f for f in range(n) if count[f] >= 4], width=p.cfg.width, height=p.cfg.height)


@functools.lru_cache(maxsize=None)
def models_case(model):
    """Test 1: one camera of `model`, frames 0..5 are the fitting ones, 6..10 are held out; seeds 1 cm and 1 degree off the truth."""
    p = synth.generate(synth.Config(models=(model,), n_frames=11, seed=21, pixel_sigma=0.1))
    held = list(range(6, 11))
    tiles = [(f - 6, c, ids, px) for (f, c, ids, px) in p.tiles if f in held]
    return _case(p, tiles, held, [perturbed(p.frame_T_wk_gt[f], f) for f in held])


@functools.lru_cache(maxsize=None)
def rig_case(models):
    """Test 2: held-out frame 0 is seen by every camera, 1 by camera 1 alone, 2 by camera 0 with 3 corners and camera 1 with 150
    (other cameras as they are), 3 by every camera again."""
    p = synth.generate(synth.Config(models=tuple(models), n_frames=10, seed=22 + len(models), pixel_sigma=0.1))
    held = [6, 7, 8, 9]
    tiles = []
    for (f, c, ids, px) in p.tiles:
        if f not in held:
            continue
        hf = f - 6
        if hf == 1 and c != 1:
            continue
        if hf == 2 and c == 0:
            sel = np.array([0, 9, len(ids) - 1])               # three corners of the grid: not collinear
            ids, px = ids[sel], px[sel]
        if hf == 2 and c == 1:
            assert len(ids) >= 150
            ids, px = ids[:150], px[:150]
        tiles.append((hf, c, ids, px))
    return _case(p, tiles, held, [perturbed(p.frame_T_wk_gt[f], 50 + f) for f in held])


RAGGED_COUNTS = (4, 63, 64, 65, 129, 190)
RAGGED_DT = (0.001, 0.003, 0.006, 0.01, 0.02, 0.035, 0.05)      # seed offsets of the seven frames, metres (and 0.1 .. 5 degrees alike)


@functools.lru_cache(maxsize=None)
def ragged_case():
    """Test 3: seven held-out frames in one launch (not a multiple of the 4 waves of a workgroup): camera 0 alone with 4, 63, 64, 65, 129
    and 190 corners, then both cameras with 190 each; every seed is off by a different amount, so the frames of one workgroup finish
    after different iteration counts."""
    p = synth.generate(synth.Config(models=("poly3", "kb4"), n_frames=8, seed=24, pixel_sigma=0.1))
    held = list(range(7))
    tiles = []
    for (f, c, ids, px) in p.tiles:
        if f >= 7:
            continue
        assert len(ids) == 190
        if f < 6:
            if c != 0:
                continue
            k = RAGGED_COUNTS[f]
            sel = np.array([0, 9, 180, 189]) if k == 4 else np.arange(k)      # (4: the grid's corners -- the first four dots are collinear)
            ids, px = ids[sel], px[sel]
        tiles.append((f, c, ids, px))
    seeds = [perturbed(p.frame_T_wk_gt[f], 80 + f, dt=RAGGED_DT[f], dr=np.deg2rad(100.0 * RAGGED_DT[f])) for f in held]
    return _case(p, tiles, held, seeds)


def three_equal_corners(ids, pix, n=130, shift=(3.0, 4.0)):
    """The first n corners of a view (copies), with corners 0, 65 and n - 1 the same target point seen at the same pixel, `shift` (5 px)
    off its detection: three bit-equal residuals, the largest of the view, in two lanes and three sweeps of a wavefront."""
    ids = np.array(ids[:n]); pix = np.array(pix[:n], dtype=np.float64)
    assert len(ids) == n
    pix[0] += shift
    ids[[65, n - 1]] = ids[0]; pix[[65, n - 1]] = pix[0]
    return ids, pix


def all_cases():
    out = [("model-" + m, models_case(m)) for m in ALL_MODELS]
    out += [("rig2", rig_case(("fov", "kb4"))), ("rig3", rig_case(("poly3", "rational6", "linear"))), ("ragged", ragged_case())]
    return out


def flat(tiles, frames=None):
    """The tiles (of the frames `frames`, renumbered 0.. in that order, or all of them) in the layout of vc_holdout_add_tiles."""
    if frames is not None:
        tiles = [(frames.index(f), c, ids, px) for (f, c, ids, px) in tiles if f in frames]
    tf = np.array([t[0] for t in tiles], dtype=np.int32); tc = np.array([t[1] for t in tiles], dtype=np.int32)
    off = np.concatenate([[0], np.cumsum([len(t[2]) for t in tiles])]).astype(np.int64)
    ids = np.concatenate([t[2] for t in tiles]).astype(np.int32) if tiles else np.zeros(0, dtype=np.int32)
    pix = np.concatenate([np.asarray(t[3], dtype=np.float64).reshape(-1, 2) for t in tiles]) if tiles else np.zeros((0, 2))
    return tf, tc, off, ids, pix


def ref_frame(case, f, cams=None):
    return hr.Frame(cams if cams is not None else case["cams"], [(c, case["grid_points"][ids], px) for (ff, c, ids, px) in case["tiles"] if ff == f])


@functools.lru_cache(maxsize=None)
def _reference(name):
    case = dict(all_cases())[name]
    out = {}
    for f in case["fitted"]:
        fr = ref_frame(case, f)
        out[f] = hr.refine(fr, case["seeds"][f])
    return out


def reference(name):
    """{held-out frame: (T_ref, info)} of a case, computed once per process."""
    return _reference(name)
