#pragma once
// vc_hostutil.hpp -- host-side helpers of the stand-alone device handles (vc_detector, vc_undistorter, vc_rectifier, vc_comparer) and of
// the calibrator's timers: opening a device, timing events, carving one allocation into aligned arrays, timing launches back to back.
// Host only, HIP and the C ABI's status codes only: the handles' translation units include this, not vc_host.hpp.
#include <hip/hip_runtime.h>
#include <cstddef>
#include "../../include/vicalib_amd.h"

namespace vch {

// makes `device` the calling thread's device.  No CPU fallback: without such a device the caller fails.
inline int open_device(int device) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess || device < 0 || device >= n || hipSetDevice(device) != hipSuccess) return VC_ERR_NO_DEVICE;
  return VC_OK;
}

// a fixed set of timing events, destroyed on every exit path
template <int N> struct EventSet {
  hipEvent_t e[N] = {};
  bool create() { for (int i = 0; i < N; ++i) if (hipEventCreate(&e[i]) != hipSuccess) return false; return true; }
  ~EventSet() { for (int i = 0; i < N; ++i) if (e[i]) (void)hipEventDestroy(e[i]); }
};

// One device allocation carved into arrays that each start on a 256-byte boundary.  The same sequence of take() calls sizes the
// allocation (base = nullptr: bytes() afterwards) and hands out the pointers (base = the allocation): the two cannot disagree.
struct Carver {
  unsigned char* base;
  size_t used = 0;
  explicit Carver(unsigned char* b = nullptr) : base(b) {}
  template <class T> T* take(size_t n) {
    T* p = base ? reinterpret_cast<T*>(base + used) : nullptr;
    used += (n * sizeof(T) + 255) & ~(size_t)255;
    return p;
  }
  size_t bytes() const { return used; }
};

// Mean time of one launch() on `stream`, `reps` of them back to back between two events, after one launch to warm up.
template <class F>
int time_back_to_back(hipStream_t stream, int reps, F&& launch, double* out_ms) {
  EventSet<2> ev;
  if (!ev.create()) return VC_ERR_NO_DEVICE;
  launch();
  bool ok = hipEventRecord(ev.e[0], stream) == hipSuccess;
  for (int r = 0; r < reps; ++r) launch();
  float ms = 0.f;
  ok = ok && hipEventRecord(ev.e[1], stream) == hipSuccess && hipEventSynchronize(ev.e[1]) == hipSuccess &&
       hipEventElapsedTime(&ms, ev.e[0], ev.e[1]) == hipSuccess && hipGetLastError() == hipSuccess;
  *out_ms = (double)ms / reps;
  return ok ? VC_OK : VC_ERR_NO_DEVICE;
}

}  // namespace vch
