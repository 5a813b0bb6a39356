// The |e|^2 launch of the CFKG passes (squared L2): its own header, so that only the translation units that launch it (ktup_cfkg.hip,
// ktup_rank_pass.hip) carry the kernel.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "ktup_common.h"

namespace ktup {
namespace {

// |e|^2 of every candidate, once per pass (squared L2 only): 16 lanes per candidate; a candidate without an entity row gets 0.
__global__ __launch_bounds__(256) void cfkg_cand_norm_kernel(const float* __restrict__ E, int64_t lde, int64_t n_ent,
                                                             const int64_t* __restrict__ cand_ids, int64_t n_cand, int d,
                                                             float* __restrict__ out) {
  const int l = threadIdx.x & 15;
  for (int64_t c = (int64_t)blockIdx.x * 16 + (threadIdx.x >> 4); c < n_cand; c += (int64_t)gridDim.x * 16) {
    const int64_t id = cand_ids ? cand_ids[c] : c;
    float s = 0.f;
    if (id >= 0 && id < n_ent) {
      const float* row = E + id * lde;
      for (int k = l; k < d; k += 16) s = fmaf(row[k], row[k], s);
    }
    s = group_sum<16>(s);
    if (l == 0) out[c] = s;
  }
}

}  // namespace
}  // namespace ktup
