"""Time of the undistortion kernels next to a plain copy of the bytes the remap moves.
640 x 480 and 1280 x 960, kb4 and poly3 (the generator's ground-truth intrinsics, scaled with the image), 64 images, destination = source size
with the intrinsics of fit_linear(alpha = 0).  Device: Undistorter.time() (HIP events on the handle's stream, launches back to back): map build,
remap of the 64 device-resident images, 65536 points.  For comparison, in the same process: a device-to-device hipMemcpyAsync of
source images + 8 B per pixel of map + destination images (what one remap launch reads and writes at the least).
   python tools/undistort_timing.py [reps]"""
import ctypes as C, os, sys; sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from vicalib_amd import lib, synth
from vicalib_amd.lib import Undistorter

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 20
N = 64
hip = lib.hip_runtime()      # the runtime the library is linked against


def ck(rc):
    assert rc == 0, rc


def copy_ms(nbytes):
    """average ms of one device-to-device hipMemcpyAsync of nbytes, `reps` back to back between two events"""
    a, b, e0, e1, ms = C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_float(0)
    ck(hip.hipMalloc(C.byref(a), nbytes)); ck(hip.hipMalloc(C.byref(b), nbytes))
    ck(hip.hipMemset(a, 1, nbytes)); ck(hip.hipEventCreate(C.byref(e0))); ck(hip.hipEventCreate(C.byref(e1)))
    ck(hip.hipMemcpyAsync(b, a, nbytes, 3, None))                       # warm-up; 3 = hipMemcpyDeviceToDevice
    ck(hip.hipEventRecord(e0, None))
    for _ in range(reps):
        ck(hip.hipMemcpyAsync(b, a, nbytes, 3, None))
    ck(hip.hipEventRecord(e1, None)); ck(hip.hipEventSynchronize(e1)); ck(hip.hipEventElapsedTime(C.byref(ms), e0, e1))
    for p in (a, b):
        hip.hipFree(p)
    hip.hipEventDestroy(e0); hip.hipEventDestroy(e1)
    return ms.value / reps


for (w, h) in ((640, 480), (1280, 960)):
    for model in ("kb4", "poly3"):
        K = np.array(synth.GT_INTRINSICS[synth.MODEL_IDS[model]], dtype=np.float64)
        K[:4] *= w / 640.0
        dl = Undistorter.fit_linear(model, K, (w, h), alpha=0.0)
        u = Undistorter(model, K, (w, h), dl)
        assert u.map()[1].all()
        t = u.time(n_images=N, reps=reps)
        moved = N * w * h + 8 * w * h + N * w * h                                     # bytes: sources + map + destinations
        cp = copy_ms(moved)
        print("%s %d x %d, %d images: map build %.4f ms; remap %.4f ms = %.1f GB/s of %.1f MB moved (%.0f images/s); copy of the same bytes %.4f ms = %.1f GB/s "
              "(read + write %.1f GB/s); remap / copy time %.2f; 65536 points %.4f ms = %.1f Mpoints/s"
              % (model, w, h, N, t["map"], t["remap"], moved / t["remap"] / 1e6, moved / 1e6, N / t["remap"] * 1e3, cp, moved / cp / 1e6, 2 * moved / cp / 1e6,
                 t["remap"] / cp, t["points"], 65536 / t["points"] / 1e3))
        u.close()
