"""Worker of the frame-sharded full-size tests (launched with torch.distributed.run, all ranks on the one GPU of the test
box; gloo carries the all-reduces of device tensors because RCCL refuses several ranks per device).

  full_size_worker.py <cfg name> <reference npz> <ranks> <store file> [<frame scale>]

The solve is sharded over <ranks> ranks.  Every worker process hosts <ranks> / WORLD_SIZE consecutive ranks, one thread and
one calibrator each: a shared GPU box admits only a few processes with the device open, fewer than the eight ranks of cfg5.
Each rank all-reduces through a gloo group of its own, set up through the file store <store file>.  Two calibrators in one process
are four streams that may share hardware queues; the sharded passes of this callback transport hand over between their two streams
through events (the device-flag hand-overs need VICALIB_AMD_SHARD_FLAG_SYNC=1 here), so that changes how the kernels are scheduled,
not which path they take.

Rank r generates frames [r N / P, (r + 1) N / P) of BASELINE <cfg> itself (native generator, nothing is shipped between the
ranks), solves the sharded problem and compares with the single-process solve the parent test stored in the npz: cost of
every LM iteration and the accept / reject sequence at 1e-7, shared parameters at 1e-7, its own frames' poses."""
import datetime
import os
import sys
import threading
import traceback
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch.distributed as dist  # noqa: E402
from vicalib_amd import synth  # noqa: E402
from vicalib_amd.lib import ViCalibrator  # noqa: E402
from vicalib_amd.parallel import FrameShardComm, frame_shard  # noqa: E402


def solve_rank(rank, world, name, ref_path, store_path, scale):
    group = dist.ProcessGroupGloo(dist.PrefixStore("full_size", dist.FileStore(store_path, world)), rank, world, datetime.timedelta(seconds=600))
    base = synth.BASELINE_CONFIGS[name]
    n_total = int(round(base.n_frames * scale))
    lo, hi = frame_shard(n_total, rank, world)
    shard = synth.generate_native(synth.Config(models=base.models, grid=base.grid, n_frames=hi - lo, imu=base.imu, first_frame=lo, extrinsics_prior=base.extrinsics_prior))
    cal = ViCalibrator(0).load_problem(shard)
    cal.SetCalibrateImu(bool(base.imu))
    comm = FrameShardComm(group=group, device="cuda:0", stream_ptr=cal.stream())
    cal.set_shard(rank, world, comm)
    cal.Solve()
    ref = np.load(ref_path)
    tg, tr = cal.trace(), ref["trace"]
    assert cal.shared_dim() == int(ref["D"]) + (9 * (world - 1) if base.imu else 0)
    assert len(tg) == len(tr), (len(tg), len(tr))
    np.testing.assert_array_equal(tg[:, 8], tr[:, 8])                      # accept / reject sequence
    np.testing.assert_array_equal(tg[:, 9], tr[:, 9])                      # stages
    np.testing.assert_allclose(tg[:, 1], tr[:, 1], rtol=1e-7)              # cost of every iteration
    for c in range(len(base.models)):
        K, T = cal.GetCamera(c)
        np.testing.assert_allclose(K, ref["K%d" % c], rtol=1e-7, atol=1e-10)
        np.testing.assert_allclose(T, ref["T%d" % c], rtol=1e-7, atol=1e-9)
    np.testing.assert_allclose(cal.GetCameraProjRMSE(), ref["rmse"], rtol=1e-7)
    if base.imu:
        np.testing.assert_allclose(cal.GetBiases(), ref["biases"], rtol=1e-6, atol=1e-10)
        np.testing.assert_allclose(cal.GetScaleFactor(), ref["scale"], rtol=1e-7)
        np.testing.assert_allclose(cal.GetGravity(), ref["gravity"], rtol=1e-7, atol=1e-10)
        assert abs(cal.time_offset() - float(ref["time_offset"])) < 1e-9
    sel = np.linspace(0, hi - lo - 1, 64).astype(int)                      # a sample of this rank's frames
    mine = np.array([cal.GetFrame(int(f))[0] for f in sel])
    np.testing.assert_allclose(mine, ref["frames"][lo + sel], rtol=1e-7, atol=1e-9)
    assert comm.calls > 0
    cal.close()
    dist.barrier(group=group)
    os.write(1, b"rank %d ok\n" % rank)        # one write: the lines of all ranks share the launcher's pipe


def main():
    name, ref_path, world, store_path = sys.argv[1], sys.argv[2], int(sys.argv[3]), sys.argv[4]
    scale = float(sys.argv[5]) if len(sys.argv) > 5 else 1.0
    proc, n_proc = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
    assert world % n_proc == 0, (world, n_proc)
    per = world // n_proc

    def run(rank):
        try:
            solve_rank(rank, world, name, ref_path, store_path, scale)
        except BaseException as e:      # noqa: BLE001
            # the peers would wait for this rank's all-reduces until the group's time-out: end the process, the launcher ends the rest
            sys.stdout.flush()
            os.write(1, ("WORKER-FAILURE rank %d: %s\n%s\n" % (rank, type(e).__name__, (str(e) + "\n" + traceback.format_exc())[:6000])).encode())
            os._exit(1)

    threads = [threading.Thread(target=run, args=(r,)) for r in range(proc * per, (proc + 1) * per)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()


if __name__ == "__main__":
    try:
        main()
    except BaseException as e:      # noqa: BLE001
        print("WORKER-FAILURE process %s: %s\n%s" % (os.environ.get("RANK"), type(e).__name__, (str(e) + "\n" + traceback.format_exc())[:6000]), flush=True)
        os._exit(1)
