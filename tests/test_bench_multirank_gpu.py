"""bench.py's multi-rank branch, executed end to end on ONE GPU (verdict r4 missing #3 / next #3): `--gpus 2 --transport gloo` starts
two ranks through torch.distributed.run, both on device 0, frames of BASELINE cfg3 split between them, the per-iteration all-reduces
through gloo and the FrameShardComm callback.  Asserts the contract of the one JSON line a driver would parse at N > 1.  This is a
functional check of the script's world > 1 code (barriers, MAX over ranks, per-rank gathers, comm object, tear-down order) -- not a
scaling measurement: no run on more than one GPU exists."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench(*extra, timeout=900):
    env = dict(os.environ)
    env.pop("WORLD_SIZE", None); env.pop("RANK", None); env.pop("LOCAL_RANK", None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), *extra], env=env, capture_output=True, text=True, timeout=timeout, cwd=ROOT)
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-3000:])
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]          # ONE JSON line, from rank 0
    return json.loads(lines[0]), r.stderr


def test_two_ranks_through_gloo_on_one_gpu():
    out, err = _bench("--gpus", "2", "--steps", "4", "--warmup", "1", "--repeats", "2", "--no-cpu-baseline", "--transport", "gloo")
    assert out["n_gpus"] == 2 and out["steps"] == 4 and out["warmup"] == 1
    assert out["metric"] == "corner_residuals_per_sec" and out["value"] > 0 and out["ms_per_step"] > 0
    assert out["config"]["frames_total"] == 2000 and out["config"]["corners_total"] == 373493      # BASELINE cfg3, both shards together
    assert out["config"]["reduced_dim"] == 29 + 9                                                    # + one separator frame
    comm = out["comm"]
    assert comm["transport"] == "gloo" and comm["communicator_size"] == 2 and comm["world_size_env"] == 2
    assert comm["ranks_agree"] is True and comm["rccl_ranks_seen"] is None      # (torch.distributed's group: every rank at its own rank)
    assert len(comm["per_rank_ms_per_step"]) == 2 and all(x > 0 for x in comm["per_rank_ms_per_step"])
    assert set(comm["allreduce_ms_per_step"]) == {"allreduce(S)", "allreduce(step scalars)"}
    assert all(v > 0 for v in comm["allreduce_ms_per_step"].values())
    assert out["roofline"] is not None and "cpu_baseline" not in out and "secondary" not in out
    # the sharded solve is the single-process solve (tests/test_sharding.py holds it to 1e-7): the complete calibration ran all stages
    assert out["complete_calibration"]["stages"] == 4 and abs(out["final_rmse_px"][0] - 0.1) < 0.01


def test_single_rank_line_is_unchanged_by_the_transport_switch():
    out, _ = _bench("--steps", "4", "--warmup", "1", "--repeats", "1", "--no-cpu-baseline", "--no-secondary")
    assert out["n_gpus"] == 1 and out["comm"] is None and out["config"]["reduced_dim"] == 29
    assert out["roofline"]["kernel"] and 0 < out["roofline"]["frac"] < 1


def test_one_rank_through_the_library_rccl_communicator_reports_what_rccl_saw():
    """VICALIB_AMD_FORCE_SHARD_PATH=1: one rank through the sharded code path with the library's own RCCL communicator -- the
    `comm` object carries what RCCL itself reports (ncclCommCount / ncclCommUserRank through vc_shard_info), not WORLD_SIZE."""
    env_keep = os.environ.get("VICALIB_AMD_FORCE_SHARD_PATH")
    os.environ["VICALIB_AMD_FORCE_SHARD_PATH"] = "1"
    try:
        out, _ = _bench("--steps", "4", "--warmup", "1", "--repeats", "1", "--no-cpu-baseline", "--no-secondary", "--workload", "cfg3", "--frames", "200")
    finally:
        if env_keep is None:
            os.environ.pop("VICALIB_AMD_FORCE_SHARD_PATH", None)
        else:
            os.environ["VICALIB_AMD_FORCE_SHARD_PATH"] = env_keep
    comm = out["comm"]
    assert comm["transport"] == "rccl" and comm["rccl_error"] is None
    assert comm["communicator_size"] == 1 and comm["rccl_ranks_seen"] == [1, 1] and comm["ranks_agree"] is True
    assert comm["allreduce_calls"] > 0


def _dump(out_dir, *extra):
    out, _ = _bench("--steps", "3", "--warmup", "1", "--repeats", "2", "--no-cpu-baseline", "--no-secondary", "--dump-outputs", str(out_dir), *extra)
    assert out["steps"] == 3
    files = {p.name[:-4]: np.load(p) for p in out_dir.iterdir()}
    assert all(p.name.endswith(".npy") for p in out_dir.iterdir())
    assert all(a.dtype == np.float64 and np.all(np.isfinite(a)) for a in files.values())
    assert sum(p.stat().st_size for p in out_dir.iterdir()) <= 64 << 20
    tr = files["trace"]
    assert tr.shape[1] == 10 and int(np.sum(tr[:, 0] > 0)) == 3 and np.all(tr[:, 9] == tr[-1, 9])     # three iterations, one stage
    assert files["state_cost"].shape == (2,) and files["state_cost"][0] > 0
    return files


def test_dump_outputs_hold_what_the_last_timed_block_computed(tmp_path):
    """--dump-outputs DIR: float64 arrays of the last timed block of cfg3 -- the solved state it ended in, its trace rows (exactly --steps
    LM iterations), the cost of that state, the IMU weights and blocks (small enough to be written whole).  Two runs with the same
    arguments write the same bits."""
    files = _dump(tmp_path / "a")
    n = 2000                                                                                   # cfg3: 2000 frames, one camera
    assert set(files) == {"trace", "state_cost", "camera0_params", "camera0_T_ck", "imu_biases", "imu_scale_factors", "gravity", "time_offset",
                          "frame_rows", "frame_poses", "frame_velocities",
                          "imu_block_rows", "imu_weights", "imu_block_hessian", "imu_block_gradient", "imu_block_cost"}
    assert files["camera0_params"].ndim == 1 and len(files["camera0_params"]) > 0 and files["camera0_T_ck"].shape == (7,)
    assert files["imu_biases"].shape == (6,) and files["imu_scale_factors"].shape == (6,) and files["gravity"].shape == (2,)
    assert files["time_offset"].shape == (1,)
    np.testing.assert_array_equal(files["frame_rows"], np.arange(n))
    assert files["frame_poses"].shape == (n, 7) and files["frame_velocities"].shape == (n, 3)
    np.testing.assert_allclose(np.linalg.norm(files["frame_poses"][:, :4], axis=1), 1.0, rtol=1e-9)      # unit quaternions
    np.testing.assert_array_equal(files["imu_block_rows"], np.arange(n - 1))
    assert files["imu_weights"].shape == (n - 1, 9, 9) and files["imu_block_hessian"].shape == (n - 1, 33, 33)
    assert files["imu_block_gradient"].shape == (n - 1, 33) and files["imu_block_cost"].shape == (n - 1,)
    again = _dump(tmp_path / "b")
    assert set(again) == set(files)
    for k in files:
        np.testing.assert_array_equal(again[k], files[k], err_msg=k)


def test_dump_outputs_vision_only_state_is_the_one_the_trace_ends_in(tmp_path):
    """cfg2 (no IMU): the reprojection cost of the dumped state, swept afresh, is the cost the trace of the block ends with (the last
    accepted row) -- the state is the one the timed iterations left on the device, not an earlier copy."""
    files = _dump(tmp_path, "--workload", "cfg2")
    assert set(files) == {"trace", "state_cost", "camera0_params", "camera0_T_ck", "camera1_params", "camera1_T_ck", "frame_rows", "frame_poses"}
    assert files["frame_poses"].shape == (500, 7)
    tr = files["trace"]
    np.testing.assert_allclose(files["state_cost"][0], tr[tr[:, 8] == 1][-1, 1], rtol=1e-9)
