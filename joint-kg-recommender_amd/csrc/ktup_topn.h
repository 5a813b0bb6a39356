// The 64-bit ranking key and the 16-lane sorted-list machinery of the evaluation kernels (ktup_rank.hip, ktup_eval.hip,
// ktup_eval_kg_fused.hip, ktup_eval_pass.hip, and through ktup_sweep_pass.h ktup_dot_pass.hip and ktup_cfkg.hip).
//        key = (order-preserving image of the fp32 score) << 32 | candidate id
// so the order is total: ascending score, ties -> lower id first.  A one-sweep pass keeps a user's sorted top-n list (one key per
// lane of a 16-lane row) in LDS and touches it only when 16 candidates are pending for it; the catalogue splits' partial lists
// are merged by topk_merge_kernel.  How a sweep keeps and renews its thresholds is its own business.
// Two list widths: the NARROW list above (topn <= TOPN_MAX = 16; every sweep), and the WIDE list of SEG = 2 or 4 such 16-key
// segments (topn <= 16 SEG <= TOPN_WIDE_MAX = 64; ktup_sweep_pass.h and ktup_eval_pass.hip): element p of a user's list is key (p >> 4) of lane
// p & 15, so a lane holds SEG keys.  Pending buffer, append and merge kernel are the same for both.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "ktup_common.h"

namespace ktup {
namespace {

constexpr uint64_t PKEY_MAX = ~0ull;   // "no key": above every real one
constexpr int TOPN_MAX = 16;           // top-n list capacity per user: one element per lane of a 16-lane row
constexpr int TOPN_WIDE_MAX = 64;      // ... of a wide list: four 16-key segments, four keys per lane
constexpr int PCAP = 32;               // pending candidates per user between two merges (a merge is due at 16; one tile adds at most 16)

// `descending` negates the score first, exactly like `per_scores = -pred` (utils/misc.py:93,180).
KTUP_DEV uint64_t topn_key(float s, bool descending, uint32_t id) {
  if (descending) s = -s;
  if (s == 0.f) s = 0.f;  // -0.0 and +0.0 compare equal in the reference's sort: one key for both
  uint32_t u = __float_as_uint(s);
  u = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
  return ((uint64_t)u << 32) | id;
}
// the (ascending) score of a key's high half; PKEY_MAX's is a NaN
KTUP_DEV float topn_key_score(uint32_t hi) { return __uint_as_float((hi & 0x80000000u) ? (hi & 0x7fffffffu) : ~hi); }

// ---- 16-lane row networks on 64-bit keys (lane j of a row = element j).  Partner j ^ K through DPP: quad_perm for 1 and 2,
// row_half_mirror . quad_perm[3,2,1,0] for 4 (7 - i then i ^ 3), row_mirror . row_half_mirror for 8.
template <int K>
KTUP_DEV uint32_t row_xor32(uint32_t v) {
  const int x = (int)v;
  if constexpr (K == 1) return (uint32_t)__builtin_amdgcn_update_dpp(x, x, 0xB1, 0xf, 0xf, false);
  else if constexpr (K == 2) return (uint32_t)__builtin_amdgcn_update_dpp(x, x, 0x4E, 0xf, 0xf, false);
  else if constexpr (K == 4) {
    const int h = __builtin_amdgcn_update_dpp(x, x, 0x141, 0xf, 0xf, false);
    return (uint32_t)__builtin_amdgcn_update_dpp(h, h, 0x1B, 0xf, 0xf, false);
  } else {
    const int m = __builtin_amdgcn_update_dpp(x, x, 0x140, 0xf, 0xf, false);
    return (uint32_t)__builtin_amdgcn_update_dpp(m, m, 0x141, 0xf, 0xf, false);
  }
}
// compare-exchange with lane j ^ K: keep the smaller key if keep_min, else the larger
template <int K>
KTUP_DEV void row_cmpx(uint64_t& v, bool keep_min) {
  const uint64_t o = ((uint64_t)row_xor32<K>((uint32_t)(v >> 32)) << 32) | row_xor32<K>((uint32_t)v);
  if ((o < v) == keep_min) v = o;
}
KTUP_DEV uint64_t row_mirror64(uint64_t v) {
  const int lo = (int)(uint32_t)v, hi = (int)(uint32_t)(v >> 32);
  return ((uint64_t)(uint32_t)__builtin_amdgcn_update_dpp(hi, hi, 0x140, 0xf, 0xf, false) << 32) |
         (uint32_t)__builtin_amdgcn_update_dpp(lo, lo, 0x140, 0xf, 0xf, false);
}
// list: a row's ascending 16 keys; cand: up to 16 more in any order (PKEY_MAX = none).  Returns the 16 smallest of the 32, ascending:
// bitonic sort of the candidates (10 exchanges), elementwise min against their mirror (a bitonic row holding the 16 smallest),
// bitonic merge (4 exchanges) -- a fixed 14 exchanges instead of one dependent ballot / bpermute round per candidate.
KTUP_DEV uint64_t row_merge16(uint64_t list, uint64_t cand, int j) {
  const bool b1 = (j & 1) == 0, b2 = (j & 2) == 0, b4 = (j & 4) == 0, b8 = (j & 8) == 0;
  row_cmpx<1>(cand, b1 == b2);
  row_cmpx<2>(cand, b2 == b4); row_cmpx<1>(cand, b1 == b4);
  row_cmpx<4>(cand, b4 == b8); row_cmpx<2>(cand, b2 == b8); row_cmpx<1>(cand, b1 == b8);
  row_cmpx<8>(cand, b8); row_cmpx<4>(cand, b4); row_cmpx<2>(cand, b2); row_cmpx<1>(cand, b1);
  const uint64_t r = row_mirror64(cand);
  uint64_t m = r < list ? r : list;
  row_cmpx<8>(m, b8); row_cmpx<4>(m, b4); row_cmpx<2>(m, b2); row_cmpx<1>(m, b1);
  return m;
}
// A row's list merged with its n <= PCAP pending candidates `row`, cut to topn keys (the four rows of a register slot at once;
// the second pass runs if any of them holds more than 16).
KTUP_DEV uint64_t row_merge_pending(uint64_t list, const uint64_t* row, int n, int topn, int j) {
  uint64_t merged = row_merge16(list, j < n ? row[j] : PKEY_MAX, j);
  if (__builtin_amdgcn_ballot_w64(n > 16)) merged = row_merge16(j < topn ? merged : PKEY_MAX, 16 + j < n ? row[16 + j] : PKEY_MAX, j);
  return j < topn ? merged : PKEY_MAX;
}
// The wide list: list[s] is this lane's key of segment s, the 16 SEG keys ascending in p = 16 s + j.  Against the ascending
// candidates C the list's LAST segment takes min(L[16 (SEG - 1) + j], C[15 - j]): with C padded by "no key" to the list's length that
// is the half-cleaner of a bitonic merge, so the 16 SEG keys now held are the smallest of the 16 SEG + 16 and form a bitonic sequence
// (ascending segments, then a last one that rises and falls, or only falls if even its first key gave way).  The bitonic merge of
// that sequence: strides 32 and 16 exchange between the lane's own keys, strides 8 to 1 are the row network on every segment.  A
// round is 10 + 4 SEG row exchanges and SEG / 2 * log2(SEG) in-lane ones: 18 + 1 with two segments, 26 + 4 with four (narrow: 14).
template <int SEG>
KTUP_DEV void row_merge16_wide(uint64_t (&list)[SEG], uint64_t cand, int j) {
  static_assert(SEG == 2 || SEG == 4, "a wide list is two or four 16-key segments");
  const bool b1 = (j & 1) == 0, b2 = (j & 2) == 0, b4 = (j & 4) == 0, b8 = (j & 8) == 0;
  row_cmpx<1>(cand, b1 == b2);                                            // the candidates' sort: row_merge16's 10 exchanges
  row_cmpx<2>(cand, b2 == b4); row_cmpx<1>(cand, b1 == b4);
  row_cmpx<4>(cand, b4 == b8); row_cmpx<2>(cand, b2 == b8); row_cmpx<1>(cand, b1 == b8);
  row_cmpx<8>(cand, b8); row_cmpx<4>(cand, b4); row_cmpx<2>(cand, b2); row_cmpx<1>(cand, b1);
  const uint64_t r = row_mirror64(cand);
  if (r < list[SEG - 1]) list[SEG - 1] = r;
#pragma unroll
  for (int h = SEG / 2; h >= 1; h >>= 1) {
#pragma unroll
    for (int s = 0; s < SEG; ++s) {
      if (s & h) continue;
      const uint64_t lo = list[s], hi = list[s | h];
      list[s] = hi < lo ? hi : lo;
      list[s | h] = hi < lo ? lo : hi;
    }
  }
#pragma unroll
  for (int s = 0; s < SEG; ++s) {
    row_cmpx<8>(list[s], b8); row_cmpx<4>(list[s], b4); row_cmpx<2>(list[s], b2); row_cmpx<1>(list[s], b1);
  }
}
// row_merge_pending for a wide list, in place (the first round's surplus keys are above every key the second round keeps: no cut
// between the rounds)
template <int SEG>
KTUP_DEV void row_merge_pending_wide(uint64_t (&list)[SEG], const uint64_t* row, int n, int topn, int j) {
  row_merge16_wide<SEG>(list, j < n ? row[j] : PKEY_MAX, j);
  if (__builtin_amdgcn_ballot_w64(n > 16)) row_merge16_wide<SEG>(list, 16 + j < n ? row[16 + j] : PKEY_MAX, j);
#pragma unroll
  for (int s = 0; s < SEG; ++s) list[s] = 16 * s + j < topn ? list[s] : PKEY_MAX;
}
// Where the candidates of a ballot go in their rows' pending buffers: lane (kq, j) belongs to row kq of the wave's four 16-lane
// rows.  No atomics: `pend`, the row's count, is replicated over its 16 lanes.
struct RowAppend {
  uint32_t lt_j; int rsh; bool rhi;
  KTUP_DEV RowAppend(int kq, int j) : lt_j((1u << j) - 1u), rsh(16 * (kq & 1)), rhi((kq & 2) != 0) {}
  // m: the wave's ballot of candidates; c: this lane is one, and key() is its key (called by candidates only).  `base`: where this
  // lane's row starts in the wave's [16][PCAP] pending buffer `pbuf`, `pend`: the row's count.
  template <class KeyFn>
  KTUP_DEV void put(uint64_t* pbuf, int base, int& pend, uint64_t m, bool c, KeyFn key) const {
    const uint32_t rb = ((rhi ? (uint32_t)(m >> 32) : (uint32_t)m) >> rsh) & 0xffffu;   // the candidates of this lane's row
    if (c) pbuf[base + pend + __popc(rb & lt_j)] = key();
    pend += __popc(rb);
  }
};

// partial lists of the splits -> the topn smallest keys per user, ids and scores (NEGATE: the key's score image negated back, for
// a sweep that ranks descending: negation is exact).  One WAVE per user: the <= 64 PER_LANE keys sit PER_LANE per lane, every lane
// ranks its keys against all of them (keys are distinct: the item id is their low half) and the keys whose rank is below topn are
// written to their slot -- no serial k-way merge, no dependent memory round trips (that version: 22 us for 6040 users).
constexpr int MERGE_T = 256;
template <int PER_LANE, bool NEGATE>
__global__ __launch_bounds__(MERGE_T) void topk_merge_kernel(const uint64_t* __restrict__ part, int64_t nq, int nsplit, int topn,
                                                             int32_t* __restrict__ top_ids, float* __restrict__ top_scores) {
  __shared__ uint64_t wk[MERGE_T / 64][64 * PER_LANE];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int64_t b = (int64_t)blockIdx.x * (MERGE_T / 64) + w;
  if (b >= nq) return;                                                    // (whole waves leave: no workgroup barrier below)
  const int per = nsplit * topn;
  const uint64_t* p = part + b * per;
  uint64_t k[PER_LANE];
  int r[PER_LANE];
  int valid = 0;
#pragma unroll
  for (int m = 0; m < PER_LANE; ++m) {
    const int idx = lane + 64 * m;
    k[m] = idx < per ? p[idx] : PKEY_MAX;
    r[m] = 0;
  }
#pragma unroll
  for (int m = 0; m < PER_LANE; ++m) {
    if (lane + 64 * m < per) wk[w][lane + 64 * m] = k[m];
    valid += __popcll(__ballot(k[m] != PKEY_MAX));
  }
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  for (int i = 0; i < per; ++i) {
    const uint64_t o = wk[w][i];
#pragma unroll
    for (int m = 0; m < PER_LANE; ++m) r[m] += o < k[m] ? 1 : 0;
  }
#pragma unroll
  for (int m = 0; m < PER_LANE; ++m) {
    if (k[m] == PKEY_MAX || r[m] >= topn) continue;
    top_ids[b * topn + r[m]] = (int32_t)(uint32_t)k[m];
    if (top_scores) {
      const float s = topn_key_score((uint32_t)(k[m] >> 32));
      top_scores[b * topn + r[m]] = NEGATE ? 0.f - s : s;
    }
  }
  if (lane >= valid && lane < topn) {                                     // fewer candidates than topn: pad
    top_ids[b * topn + lane] = -1;
    if (top_scores) top_scores[b * topn + lane] = 0.f;
  }
}

}  // namespace
}  // namespace ktup
