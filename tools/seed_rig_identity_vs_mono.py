"""Does the rig seed cure the slow start of the 8-camera rig?  The generator's cfg5 rig (fov, kb4 x 4; 0.42 m wide next to a 0.25 m target) at
200 frames, vision only, through the command line: once from the engine's identity extrinsics, once with -seed_rig mono; both with
-seed_focal -pnp_device.  Prints the iterations, the end of the run (exit status, the tool's verdict line) and the wall time of the whole run
and of the mono stage.  Nothing is asserted: the figures go into DESIGN 4.21 and profiles/seed_rig_timing.txt.
   python tools/seed_rig_identity_vs_mono.py [n_frames]"""
import os, re, subprocess, sys, tempfile, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from vicalib_amd import synth

n = int(sys.argv[1]) if len(sys.argv) > 1 else 200
p = synth.generate(synth.Config(models=("fov", "kb4") * 4, n_frames=n, seed=5))
with tempfile.TemporaryDirectory() as d:
    files, _ = synth.write_dataset(p, d)
    base = [os.path.join(ROOT, "vicalib_amd", "vicalib"), "-cam", "detections://" + ",".join(files), "-models", ",".join(p.cfg.models), "-nocalibrate_imu", "-grid_preset", "small",
            "-seed_focal", "-pnp_device", "-output", os.path.join(d, "cameras.xml")]
    for name, extra in (("identity", []), ("-seed_rig mono", ["-seed_rig", "mono"])):
        t0 = time.time()
        r = subprocess.run(base + extra, cwd=d, capture_output=True, text=True, timeout=900)
        wall = time.time() - t0
        it = re.search(r"iterations: (\d+)\s+mse: (\S+)\s+solve time: (\S+) s", r.stdout)
        mono = re.search(r"cameras calibrated alone in (\S+) s", r.stderr)
        rmse = re.findall(r"reprojection RMSE: (\S+) px", r.stdout)
        verdict = [l.split(" -> ")[0] for l in (r.stdout + r.stderr).splitlines() if "calibration" in l.lower() and ("succe" in l.lower() or "fail" in l.lower())]
        print("%s: exit status %d, %s iterations, mse %s, solve %s s, whole run %.2f s, mono stage %s s; RMSE per camera %s; %s"
              % (name, r.returncode, it.group(1) if it else "?", it.group(2) if it else "?", it.group(3) if it else "?", wall, mono.group(1) if mono else "-", " ".join(rmse),
                 "; ".join(verdict[-2:])))
        for l in r.stderr.splitlines():
            if "seed_rig" in l or l.startswith("W ") or l.startswith("E ") or l.startswith("F "):
                print("   ", l)
