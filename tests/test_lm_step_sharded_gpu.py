"""One held LM step of the frame-sharded pass against a dense reference solve of the whole problem (tests/lm_step_ref.py), and the
read-outs of a sharded visual-inertial rank.

With the IMU every rank r > 0 moves its first frame into the reduced system as 9 separator columns (D = D0 + 9 (P - 1)), and rank r - 1
keeps a ghost copy of it.  test_lm_step_gpu.py covers the single-process pass; here each case runs its P ranks as threads of one child
process (tests/lm_step_sharded_worker.py), one case at a time, and checks at radii 1, 1e4 and 1e8:
  - the width of the reduced system and, with the IMU, the forms of the pass each rank ran;
  - the ranks' IMU weights, in block order, against the single-process calibrator's at the same state (1e-12);
  - the all-reduced S / g_red of linearize() against the dense Schur complement of the whole Hessian with the separators kept;
  - the damping of the shared parameters, of every separator at its columns and of every rank's own frames (1e-12);
  - delta_s: the same bits on every rank, and within test_lm_step_gpu's bound of the reference step, shared and separator parts;
  - the trial state of every rank's own frames, the cameras and the IMU parameters, the shared part the same bits on every rank.
Each case prints kappa(M~), the bound and the largest error / bound at radius 1.  Two more children check that no read-out writes past
the size the header documents, and that a reduced system one column wider than k_reduced's LDS image holds (D = 179 on gfx950) is
refused at upload."""
import os
import subprocess
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

import lm_step_sharded_worker as w      # noqa: E402

pytestmark = pytest.mark.gpu


def _child(what, tmp_path, env=None, timeout=600):
    """The worker for one case, in a process of its own (event hand-overs: several calibrators share the process's queues)."""
    e = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0", VICALIB_AMD_FLAG_SYNC="0")
    e.update(env or {})
    out = subprocess.run([sys.executable, os.path.join(HERE, "lm_step_sharded_worker.py"), what, str(tmp_path)], env=e,
                         capture_output=True, text=True, timeout=timeout)
    print(out.stdout)
    fail = out.stdout.find("WORKER-FAILURE")
    assert out.returncode == 0 and fail < 0, (out.stdout[fail:fail + 7000] if fail >= 0 else out.stdout[-3000:] + out.stderr[-3000:])
    assert ("ok " + what) in out.stdout
    return out


@pytest.mark.parametrize("name", list(w.CASES))
def test_sharded_lm_step_matches_dense_reference_solve(name, tmp_path):
    _child(name, tmp_path, env=w.CASES[name]["env"], timeout=900)


def test_sharded_readouts_write_their_documented_sizes(tmp_path):
    _child("readouts", tmp_path)


def test_reduced_system_one_past_the_lds_limit_is_refused(tmp_path):
    """D = 180 refused on every rank before any launch of k_reduced, then D = 92 taken by the same calibrators.  Together with the
    D = 179 case above this pins the limit reduced_fits derives from the runtime's report: if the compiler moves it, one of the two fails."""
    out = _child("limit", tmp_path)
    assert out.stderr.count("a reduced system of 180 shared parameters") == 8, out.stderr[-3000:]
