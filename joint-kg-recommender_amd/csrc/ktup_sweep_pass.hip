// The filter bitmap of a one-sweep top-n pass (ktup_sweep_pass.h), compiled here once for both passes.
#include "ktup_sweep_pass.h"

namespace ktup {

__global__ __launch_bounds__(256) void sweep_filter_zero_kernel(uint32_t* __restrict__ bm, int64_t n) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) bm[i] = 0u;
}
// one wave per user of the pass
__global__ __launch_bounds__(256) void sweep_filter_bits_kernel(const int64_t* __restrict__ off, const int32_t* __restrict__ ids, int64_t nq,
                                                                int64_t n, uint32_t* __restrict__ bm, int64_t words) {
  const int lane = threadIdx.x & 63;
  for (int64_t b = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); b < nq; b += (int64_t)gridDim.x * 4) {
    const int64_t f1 = off[b + 1];
    for (int64_t f = off[b] + lane; f < f1; f += 64) {
      const int64_t id = ids[f];
      if (id >= 0 && id < n) atomicOr(bm + b * words + (id >> 5), 1u << (id & 31));
    }
  }
}

int sweep_filter_bits(const int64_t* off, const int32_t* ids, int64_t nq, int64_t n, uint32_t* bm, int64_t words, hipStream_t st,
                      const char* name) {
  const int64_t nw = nq * words;
  hipLaunchKernelGGL(sweep_filter_zero_kernel, dim3((unsigned)min((nw + 255) / 256, (int64_t)4096)), dim3(256), 0, st, bm, nw);
  if (int rc = check_launch(name)) return rc;
  hipLaunchKernelGGL(sweep_filter_bits_kernel, dim3((unsigned)min((nq + 3) / 4, (int64_t)4096)), dim3(256), 0, st, off, ids, nq, n, bm, words);
  return check_launch(name);
}

}  // namespace ktup
