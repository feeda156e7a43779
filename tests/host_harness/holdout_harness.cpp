// Host build of the frame selection behind -holdout_every (vicalib_amd/csrc/vc_holdout_select.hpp) for tests/test_holdout_cpu.py.
#include "../../vicalib_amd/csrc/vc_holdout_select.hpp"

extern "C" void vch_held(long long n, int every, int* out) {
  for (long long i = 0; i < n; ++i) out[i] = vc::holdout_is_held(i, every) ? 1 : 0;
}
extern "C" long long vch_num_held(long long n, int every) { return vc::holdout_num_held(n, every); }
extern "C" int vch_every_ok(long long n, int every) { return vc::holdout_every_ok(n, every) ? 1 : 0; }
