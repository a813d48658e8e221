// k1_lookups_harness.hip -- TEST INFRASTRUCTURE: the tile search's branch-free lookups (dev_predict.h, dev_common.h, unchanged) on every argument of
// k1_lookups_domain.h, one argument per lane in one launch: thread i evaluates argument i, so the lanes of a 16-lane row and the rows of a wave hold different
// arguments -- what the earlier switch / if forms met with divergent decision trees.  Built by tests/helpers/kernel_build.py with the product's flags.
#include <hip/hip_runtime.h>
#include "k1_lookups_domain.h"

__global__ __launch_bounds__(64) void k1l_kernel(int *out, int n) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  out[i] = k1l_new(k1l_arg(i));
}

extern "C" int k1l_total(void) { return K1L_TOTAL; }

// out: k1l_total() values.  Returns 0, -1 for a count that is not the domain's (nothing is launched then), -10 for a HIP error.
extern "C" int k1l_run(int *out, int n) {
  if (!out || n != K1L_TOTAL) return -1;
  int *d = nullptr;
  if (hipMalloc(&d, (size_t)n * sizeof(int)) != hipSuccess) return -10;
  int rc = 0;
  if (hipMemset(d, 0xff, (size_t)n * sizeof(int)) != hipSuccess) rc = -10;
  if (rc == 0) {
    hipLaunchKernelGGL(k1l_kernel, dim3((n + 63) / 64), dim3(64), 0, 0, d, n);
    if (hipGetLastError() != hipSuccess || hipDeviceSynchronize() != hipSuccess) rc = -10;
  }
  if (rc == 0 && hipMemcpy(out, d, (size_t)n * sizeof(int), hipMemcpyDeviceToHost) != hipSuccess) rc = -10;
  (void)hipFree(d);
  return rc;
}
