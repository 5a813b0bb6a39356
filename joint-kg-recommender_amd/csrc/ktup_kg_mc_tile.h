// The score-forming device code the squared-L2 matrix-core KG routes share: the chunked score kernel (ktup_eval_mc.hip
// pairs_kg_l2_mc_kernel, TransE / TransR) and the pass without the score matrix (ktup_eval_kg_fused.hip: list kernel and sweep).
// ONE copy => the same MFMA k-order (whole groups of four, then the b32 tail at d % 16 == 4) and the same epilogue expression on
// the same operands, so a (key, candidate) score has the same bits on either route.
#pragma once
#include "ktup_common.h"
#include "ktup_lane_swap.h"

namespace ktup {

// one 16 x 16 (keys x candidates) product: qa = the lane's query row + kq, cb = its candidate row + kq (float4 chunks, kq = lane / 16);
// KGF whole k groups of 16 coordinates, TAIL1: one more chunk through a single b32-operand MFMA
template <int KGF, bool TAIL1>
KTUP_DEV v4 kg_tile_dot1(const v4* qa, const v4* cb) {
  v4 ce = (v4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int g = 0; g < KGF; ++g) {
    const v4 ac = qa[4 * g], be = cb[4 * g];
#pragma unroll
    for (int c = 0; c < 4; ++c) ce = __builtin_amdgcn_mfma_f32_16x16x4f32(ac[c], be[c], ce, 0, 0, 0);
  }
  if (TAIL1) {
    const int kq = (threadIdx.x & 63) >> 4;
    const float qf = (reinterpret_cast<const float*>(qa - kq + 4 * KGF) + kq)[0];
    const float be = (reinterpret_cast<const float*>(cb - kq + 4 * KGF) + kq)[0];
    ce = __builtin_amdgcn_mfma_f32_16x16x4f32(qf, be, ce, 0, 0, 0);
  }
  return ce;
}

// |c - e|^2 from the product: cc = |c|^2, en = |e|^2 (TransR: |c|^2 of the unfolded query and |M_r e|^2 from the pass's table)
KTUP_DEV float kg_l2_score(float ce, float cc, float en) { return fmaf(-2.f, ce, cc + en); }

}  // namespace ktup
