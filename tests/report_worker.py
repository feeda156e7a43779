"""Worker of tests/test_report_gpu.py::test_two_ranks_report_their_own_frames (launched with torch.distributed.run, two ranks on one GPU
over gloo): the residual report is rank-local -- the ranks' corner and IMU rows concatenated are the single-handle report, their error
maps add up to its maps.  Same state on both sides, no solve."""
import os
import sys
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import torch  # noqa: E402,F401
import torch.distributed as dist  # noqa: E402
from vicalib_amd import synth  # noqa: E402
from vicalib_amd.parallel import FrameShardComm, frame_shard  # noqa: E402
from dist_worker import load_slice, _guarded  # noqa: E402

N_TOTAL = 40
MODELS = ("kb4", "poly3")


def _state(cal, p):
    gt = p.imu_gt
    cal.SetOptimizationFlags(True, True, False, True)
    cal.SetBiases(np.concatenate([gt["bg"], gt["ba"]]) * 0.8); cal.SetScaleFactor(np.concatenate([gt["sg"], gt["sa"]]))
    cal.SetTimeOffset(0.002); cal.SetGravity(np.array([0.01, -0.02]))
    return cal


def main():
    from vicalib_amd.lib import ViCalibrator
    from test_report_gpu import _numpy_maps, EPS
    rank = int(os.environ["RANK"]); world = int(os.environ["WORLD_SIZE"])
    dist.init_process_group("gloo", rank=rank, world_size=world)
    full = synth.generate(synth.Config(models=MODELS, n_frames=N_TOTAL, imu=True, seed=5))
    lo, hi = frame_shard(N_TOTAL, rank, world)
    cal = _state(load_slice(ViCalibrator(0), full, lo, hi), full)
    comm = FrameShardComm(device="cuda:0", stream_ptr=cal.stream())
    cal.set_shard(rank, world, comm)
    rep = cal.report()
    assert len(rep["imu"]["flags"]) == cal.num_imu_blocks() == (hi - lo - 1) + (1 if rank + 1 < world else 0)
    mine = dict(r=rep["r"], frame=rep["frame"] + lo, camera=rep["camera"], flags=rep["flags"], maps=rep["maps"],
                whitened=rep["imu"]["whitened"], unwhitened=rep["imu"]["unwhitened"], imu_flags=rep["imu"]["flags"],
                view_frame=rep["views"]["frame"] + lo, view_sq=rep["views"]["sum_sq"], view_worst=rep["views"]["worst_corner"])
    parts = [None] * world
    dist.all_gather_object(parts, mine)
    ref = _state(ViCalibrator(0).load_problem(full), full)
    one = ref.report()
    cat = lambda k: np.concatenate([q[k] for q in parts])      # noqa: E731
    for k in ("r", "frame", "camera", "flags"):
        np.testing.assert_array_equal(cat(k), one[k])
    np.testing.assert_array_equal(cat("view_frame"), one["views"]["frame"])
    np.testing.assert_array_equal(cat("view_sq"), one["views"]["sum_sq"])
    first = np.cumsum([0] + [len(q["r"]) for q in parts])[:-1]
    np.testing.assert_array_equal(np.concatenate([q["view_worst"] + first[i] for i, q in enumerate(parts)]), one["views"]["worst_corner"])
    assert len(one["imu"]["flags"]) == N_TOTAL - 1
    for k in ("whitened", "unwhitened"):
        np.testing.assert_allclose(cat(k), one["imu"][k], rtol=1e-12, atol=0.0)      # (the block across the boundary comes from rank 0)
    np.testing.assert_array_equal(cat("imu_flags"), one["imu"]["flags"])
    summed = sum(q["maps"] for q in parts)
    pix = np.concatenate([t[3] for t in full.tiles])
    maps, mabs = _numpy_maps(one, pix, full.cfg.width, full.cfg.height, len(MODELS))
    np.testing.assert_array_equal(summed[..., 0], one["maps"][..., 0])
    assert np.all(np.abs(summed[..., 1:] - one["maps"][..., 1:]) <= maps[..., :1] * EPS * mabs[..., 1:])      # n_cell * eps * sum |x_i|
    dist.barrier()
    dist.destroy_process_group()
    print("rank", rank, "ok")


if __name__ == "__main__":
    _guarded(main)
