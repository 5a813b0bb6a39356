// What the one-launch KG training steps share: kg_step_kernel (ktup_train_step.hip), kg_step_rows_kernel (ktup_shard_kg.hip) and
// transd_step_kernel (ktup_transd_step.hip).  A lane group of GL = 16 / 32 / 64 lanes owns "pair" k = the positive triple k and its
// corrupted twin k + B and holds their rows in registers, one float4 per lane.  Here live, ONCE: the walk over the pairs, the
// TransE / TransH arithmetic of a pair, normLoss over rows in registers, the gradient scatter's two forms, the workgroup tail, the
// lane-group dispatch of the launchers and the host check of such rows.  Each kernel keeps its own loads, prefetch and stores.
#pragma once
#include <initializer_list>
#include <type_traits>

#include "ktup_common.h"

namespace ktup {

// ---- host side -------------------------------------------------------------------------------
// f(std::integral_constant<int, GL>) with the narrowest lane group that holds a row of nch float4 chunks
template <typename F>
inline int with_lane_group(int nch, F f) {
  if (nch <= 16) return f(std::integral_constant<int, 16>{});
  if (nch <= 32) return f(std::integral_constant<int, 32>{});
  return f(std::integral_constant<int, 64>{});
}

// "float4 lane-group rows": d floats = at most 64 float4 chunks, every pitch a whole number of chunks, every table 16-byte aligned
// (a null pointer, i.e. a table the call does not use, passes)
inline bool lane_group_rows_ok(int d, std::initializer_list<int64_t> pitches, std::initializer_list<const void*> tables) {
  if (d <= 0 || d % 4 || d > 256) return false;
  for (int64_t ld : pitches) if (ld % 4) return false;
  for (const void* p : tables) if (!aligned16(p)) return false;
  return true;
}

// ---- device side -----------------------------------------------------------------------------
// First pair and stride of a lane group in a 256-thread workgroup.  serial (option `deterministic`): ONE lane group of one workgroup
// walks every pair, so that each gradient cell receives its adds in program order (the sums of float atomics from several waves
// depend on the order they land in); the launch then has one workgroup.
template <int GL>
struct PairWalk {
  int64_t k0, step;
  KTUP_DEV PairWalk(int serial, int64_t B)
      : k0(serial ? (threadIdx.x < GL ? 0 : B) : (int64_t)blockIdx.x * (256 / GL) + threadIdx.x / GL),
        step(serial ? 1 : (int64_t)gridDim.x * (256 / GL)) {}
};

// normLoss (utils/loss.py:21-23) of N rows in registers: sum max(|x|^2 - 1, 0) to `part` (lane 0), 2 g1 x to the gradient of a row
// with |x|^2 - 1 > 0; hit[i] (optional) is set for such a row
template <int GL, int N>
KTUP_DEV void norm_loss_rows(const float4 (&x)[N], float g1, int lane, float& part, float4 (&g)[N], bool* hit = nullptr) {
#pragma unroll
  for (int i = 0; i < N; ++i) {
    const float s = group_sum<GL>(dot4(x[i], x[i]));
    if (s - 1.f > 0.f) {
      g[i] = fma4(2.f * g1, x[i], g[i]);
      if (hit) hit[i] = true;
    }
    if (lane == 0) part += fmaxf(s - 1.f, 0.f);
  }
}

// The TransE / TransH pair: e = [ph, pt, nh, nt], rr / ww = the relation and norm rows of the positive triple and of its twin.
// Adds to part[4] = margin sum, orth, normE, normR (lane 0) and leaves the gradients of all eight rows, regularisers included
// (regs: bit 0 orthogonalLoss(rel, norm) rows, bit 1 normLoss(entity rows), bit 2 normLoss(relation rows)).
template <int GL, bool TRANSH>
KTUP_DEV void kg_pair_math(const float4 (&e)[4], const float4 (&rr)[2], const float4 (&ww)[2], bool l1, float margin, float g1, int regs,
                           int lane, float (&part)[4], float4 (&ge)[4], float4 (&gr)[2], float4 (&gw)[2]) {
  // ---- forward of both triples (transH.py:58-71 / transE.py:51-63)
  float dh[2] = {0.f, 0.f}, dt[2] = {0.f, 0.f}, sc[2];
  float4 z[2];
#pragma unroll
  for (int x = 0; x < 2; ++x) {
    const float4 hh = e[2 * x], tt = e[2 * x + 1];
    if (TRANSH) {
      dh[x] = group_sum<GL>(dot4(hh, ww[x]));
      dt[x] = group_sum<GL>(dot4(tt, ww[x]));
      const float4 ph = fma4(-dh[x], ww[x], hh), pt = fma4(-dt[x], ww[x], tt);
      z[x] = (ph + rr[x]) - pt;
    } else {
      z[x] = (hh + rr[x]) - tt;
    }
    sc[x] = group_sum<GL>(dist4(z[x], l1));
  }
  // ---- marginLoss (utils/loss.py:8-16): sum_k max(pos - neg + margin, 0)
  const float diff = sc[0] - sc[1];
  const bool act = diff + margin > 0.f;
  if (lane == 0) part[0] += fmaxf(diff + margin, 0.f);
  const float gs[2] = {act ? g1 : 0.f, act ? -g1 : 0.f};
  // ---- backward of both triples
#pragma unroll
  for (int x = 0; x < 2; ++x) {
    const float4 gz = gs[x] * ddist4(z[x], l1);
    if (TRANSH) {
      const float aw = group_sum<GL>(dot4(gz, ww[x]));
      const float sq = dh[x] - dt[x];
      const float4 q = e[2 * x] - e[2 * x + 1];
      ge[2 * x] = fma4(-aw, ww[x], gz);                          // gh
      ge[2 * x + 1] = -1.f * ge[2 * x];                          // gt
      gw[x] = fma4(-aw, q, (-sq) * gz);                          // gw
    } else {
      ge[2 * x] = gz;
      ge[2 * x + 1] = -1.f * gz;
      gw[x] = f4zero();
    }
    gr[x] = gz;
  }
  // ---- the regularisers of the rows in registers
  if (regs & 2) norm_loss_rows<GL>(e, g1, lane, part[2], ge);
  if (TRANSH && (regs & 1)) {         // orthogonalLoss(rel rows, norm rows): sum (w.r)^2 / |r|^2  (utils/loss.py:18-19)
#pragma unroll
    for (int x = 0; x < 2; ++x) {
      const float dot = group_sum<GL>(dot4(rr[x], ww[x])), nr = group_sum<GL>(dot4(rr[x], rr[x]));
      const float c1 = g1 * 2.f * dot / nr, c2 = g1 * 2.f * dot * dot / (nr * nr);
      gr[x] = gr[x] + fma4(-c2, rr[x], c1 * ww[x]);
      gw[x] = fma4(c1, rr[x], gw[x]);
      if (lane == 0) part[1] += dot * dot / nr;
    }
  }
  if (regs & 4) norm_loss_rows<GL>(rr, g1, lane, part[3], gr);
}

// ---- the scatter of an example's gradients.  A kernel writes its list of (cell, gradient, condition) ONCE, as a generic lambda over
// the adder, and calls it with RowAdd<true> (the norm is tracked: ktup_common.h) or RowAdd<false>.  The adder returns what the fold
// needs; the list folds with gain() after its last add, so no returned value is consumed before every add of the example was issued.
// A row whose condition is false gets no atomic and folds to 0.
struct RowAdded { float4 old, v; bool hit; };
KTUP_DEV float gain(const RowAdded& r) { return r.hit ? sq_gain4(r.old, r.v) : 0.f; }
template <bool TRACK>
struct RowAdd {
  static constexpr bool track = TRACK;
  KTUP_DEV RowAdded operator()(float* cell, float4 v, bool cond = true) const {
    RowAdded r{f4zero(), v, TRACK && cond};
    if (cond) {
      if (TRACK) r.old = atomic_add4_old(cell, v);
      else atomic_add4(cell, v);
    }
    return r;
  }
};

// ---- the tail of a 256-thread step workgroup: the four loss values and the tracked squared norm (gnorm may be null) as wave sums ->
// one atomic per workgroup and slot; a slot that stayed 0 is not written
KTUP_DEV void step_tail(const float (&part)[4], float ssq, double* gnorm, int gset, float* loss) {
  __shared__ float red[4][5];
  const bool track = gnorm != nullptr;
#pragma unroll
  for (int s = 0; s < 4; ++s) {
    const float v = group_sum<64>(part[s]);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6][s] = v;
  }
  if (track) {
    ssq = group_sum<64>(ssq);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6][4] = ssq;
  }
  __syncthreads();
  if (track && threadIdx.x == 64) gnorm_add(gnorm, gset, ((double)red[0][4] + (double)red[1][4]) + ((double)red[2][4] + (double)red[3][4]));
  if (threadIdx.x < 4) {
    const float v = (red[0][threadIdx.x] + red[1][threadIdx.x]) + (red[2][threadIdx.x] + red[3][threadIdx.x]);
    if (v != 0.f) atomicAdd(loss + threadIdx.x, v);
  }
}

}  // namespace ktup
