// Host build of the residual report's binning (vicalib_amd/csrc/vc_report_bins.hpp) for tests/test_report_cpu.py.
#include "../../vicalib_amd/csrc/vc_report_bins.hpp"

extern "C" void vcr_cells(const double* x, int n, int bins, int extent, int* out) {
  for (int i = 0; i < n; ++i) out[i] = vc::report_cell(x[i], bins, extent);
}
