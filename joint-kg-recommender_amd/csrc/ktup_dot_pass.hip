// K11 + K17 fused for a whole evaluation pass of the inner-product recommenders (BPRMF, FM, CKE, coFM): all-item scores
//     score(b, j) = (U[u_b] . I[j] + user_add[b]) + item_add[j]
// AND the filtered top-n of every user in ONE sweep that never writes the (users x items) score matrix.
//
// Reference: bprmf.py:51-54 / fm.py:69-80 / CKE.py:142-153 / cofm.py:127-141 produce a (B x N) matrix per batch of 512 users,
// which utils/misc.py:186-248 copies to the host, argsorts and walks.  The per-batch route of this build keeps that shape on the
// device (ktup_eval_bprmf_scores, two torch adds, ktup_eval_topk_filtered, ktup_eval_rec_metrics per batch).  Here:
//   * scores: v_mfma_f32_16x16x4_f32 with k ascending -- fp32 in, fp32 accumulate, bit for bit the fmaf chain of K11
//     (bprmf_eval_kernel) -- then the two separately rounded adds, so the scores and with them the ranked lists are the per-batch
//     route's bits;
//   * a workgroup owns 64 users (4 waves x 16) and a contiguous split of the catalogue.  A wave keeps its 16 users' rows in
//     REGISTERS for the whole pass (one float per lane and 4 k); items stream through a double-buffered LDS stage (rows at an odd
//     float4 pitch: the B operand reads of a 16-item tile hit 64 different banks; the item's additive term rides in the row's last
//     slot) that the next stage's global loads refill under the MFMAs.  Every 16-item tile of a stage has an accumulator of its
//     own: independent MFMA chains per wave;
//   * ranking: as in ktup_eval_pass.hip -- a user's sorted top-n list (64-bit keys = order-preserving image of the NEGATED score
//     << 32 | item id: descending score, ties -> lower id, the order of ktup_rank.hip with descending = 1) lives in the wave's LDS
//     and is touched only when 16 candidates are pending for it.  A score is a candidate if it beats the user's n-th score (one
//     float compare; the keys decide equality, NaNs and a list that is still short) and its bit in the pass's filter bitmap (built
//     once per pass from the CSR lists, read from L2 by candidates only) is clear;
//   * the splits' partial lists are merged by a last, tiny launch.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "ktup_common.h"
#include "ktup_lane_swap.h"
#include "ktup_topn.h"

namespace ktup {
namespace {

constexpr int NSPLIT_MAX = 32;   // catalogue splits: NSPLIT_MAX * TOPN_MAX keys per user is what the merge holds, eight per lane
constexpr int MERGE_PER_LANE = NSPLIT_MAX * TOPN_MAX / 64;
constexpr size_t WAVE_LDS = (size_t)16 * PCAP * 8 + (size_t)16 * 16 * 8;   // pending rows | lists

// The filter lists of a pass as bits, once per pass: bm[b * words + (id >> 5)] bit (id & 31), one wave per user of u_ids.
__global__ __launch_bounds__(256) void dot_filter_zero_kernel(uint32_t* __restrict__ bm, int64_t n) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) bm[i] = 0u;
}
__global__ __launch_bounds__(256) void dot_filter_bits_kernel(const int64_t* __restrict__ off, const int32_t* __restrict__ ids, int64_t nq,
                                                              int64_t n_items, uint32_t* __restrict__ bm, int64_t words) {
  const int lane = threadIdx.x & 63;
  for (int64_t b = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); b < nq; b += (int64_t)gridDim.x * 4) {
    const int64_t f1 = off[b + 1];
    for (int64_t f = off[b] + lane; f < f1; f += 64) {
      const int64_t id = ids[f];
      if (id >= 0 && id < n_items) atomicOr(bm + b * words + (id >> 5), 1u << (id & 31));
    }
  }
}

struct DotArgs {
  const float* U; int64_t ldu;
  const float* I; int64_t ldi;
  int d, ivec;                          // ivec: item rows are whole, 16-byte aligned float4 (else element by element)
  const int64_t* u_ids; int64_t nq, n_items;
  const float *user_add, *item_add;     // NULL = none
  const uint32_t* bm; int64_t bm_words; // the filter bits [nq][bm_words]; NULL = no filter
  int topn, nsplit; int64_t split_items;
  uint64_t* part;                       // [nq][nsplit][topn] partial lists
};

// KS: 4-wide k steps (d <= 4 KS; the padding multiplies zeros: fma(0, 0, acc) = acc, and a chain that starts at +0 never holds -0)
template <int KS>
struct DotGeom {
  static constexpr int ST = KS > 32 ? 32 : 64;       // items per stage
  static constexpr int NSUB = ST / 16;               // 16-item tiles per stage = accumulators per wave
  static constexpr int CPR = KS + 1;                 // float4 slots per item row: KS operand quads + {item_add, 0, 0, 0}
  static constexpr int ROW4 = CPR | 1;               // the row's float4 pitch in LDS: odd
  static constexpr int STG = ST * ROW4;              // float4 per stage buffer
  static constexpr int SLOTS = ST * KS;              // operand quads a stage loads
  static constexpr int NPRE = (SLOTS + 255) / 256;   // float4 per thread in flight for the next stage
  static constexpr size_t LDS = (size_t)2 * STG * 16 + 4 * WAVE_LDS;
};

template <int KS, bool VEC>
__global__ __launch_bounds__(256, 2) void dot_pass_kernel(DotArgs a) {
  using G = DotGeom<KS>;
  constexpr int ST = G::ST, NSUB = G::NSUB, ROW4 = G::ROW4, STG = G::STG, SLOTS = G::SLOTS, NPRE = G::NPRE;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  v4* Xb = reinterpret_cast<v4*>(smem);                                   // [2][STG] item stages
  const int tid = threadIdx.x, lane = tid & 63, kq = lane >> 4, j = lane & 15;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  uint64_t* pbuf = reinterpret_cast<uint64_t*>(smem + (size_t)2 * STG * 16 + (size_t)w * WAVE_LDS);   // [16][PCAP] pending candidates
  uint64_t* tk = pbuf + 16 * PCAP;                                        // [16][16] the users' sorted lists (touched by merges only)
  const int64_t ub = (int64_t)(blockIdx.x / (unsigned)a.nsplit);
  const int sp = (int)(blockIdx.x - (unsigned)ub * (unsigned)a.nsplit);
  const int64_t u0 = ub * 64 + 16 * w;
  const int64_t i_lo = (int64_t)sp * a.split_items;
  const int64_t i_hi = min(a.n_items, i_lo + a.split_items);
  const int topn = a.topn, d = a.d;
  for (int idx = lane; idx < 16 * 16; idx += 64) tk[idx] = PKEY_MAX;
  // A operands of the whole pass: lane (kq, j) holds U[user j][4 s + kq] for every k step s
  float av[KS];
  {
    const bool ok = u0 + j < a.nq;
    const float* urow = a.U + (ok ? a.u_ids[u0 + j] : 0) * a.ldu;
#pragma unroll
    for (int s = 0; s < KS; ++s) av[s] = urow[min(4 * s + kq, d - 1)];     // (unconditional, from clamped addresses: all in flight together)
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int s = 0; s < KS; ++s) av[s] = (ok && 4 * s + kq < d) ? av[s] : 0.f;
  }
  float uadd[4] = {0.f, 0.f, 0.f, 0.f};
  uint64_t thr[4];                                                        // the users' n-th keys (rows past the end: nothing is ever below)
  // ... and their scores: a score above is a candidate, one below is not -- one float compare per score; an equal score, a NaN on
  // either side (the threshold of a list that is still short is one) or a zero of the other sign goes through the 64-bit key
  // compare, so the order is that of the keys in every case
  float thrf[4];
  int pend[4] = {0, 0, 0, 0};
#pragma unroll
  for (int reg = 0; reg < 4; ++reg) {
    const int64_t ur = u0 + 4 * kq + reg;
    thr[reg] = ur < a.nq ? PKEY_MAX : 0ull;
    thrf[reg] = ur < a.nq ? __uint_as_float(0x7fffffffu) : __builtin_inff();
    if (a.user_add && ur < a.nq) uadd[reg] = a.user_add[ur];
  }
  // ---- the stage loads: slot e of a stage = operand quad c of item row r (r = e / KS); rows past the table's end re-read its last
  // row (their items are masked out below, the operands only have to be there).  Straight-line code: every load is unconditional
  // from a clamped address and zeroed by a select where it is padding, so that all loads of a stage are in flight together (with
  // a branch per slot the compiler waited for each load before the next: 17 round trips per stage).  The item's additive term
  // is loaded by the first ST threads.
  v4 pre[NPRE];
  float pre_add = 0.f;
  auto fetch = [&](int64_t row0) __attribute__((always_inline)) {
#pragma unroll
    for (int k = 0; k < NPRE; ++k) {
      const int e = min(tid + 256 * k, SLOTS - 1);
      const int r = e / KS, c = e - r * KS;
      const int64_t item = min(row0 + r, a.n_items - 1);
      const float* row = a.I + item * a.ldi;
      if constexpr (VEC) {
        pre[k] = *reinterpret_cast<const v4*>(row + min(4 * c, d - 4));
      } else {
#pragma unroll
        for (int q = 0; q < 4; ++q) pre[k][q] = row[min(4 * c + q, d - 1)];
      }
    }
    if (a.item_add) pre_add = a.item_add[min(row0 + min(tid, ST - 1), a.n_items - 1)];
  };
  auto stash = [&](int buf) __attribute__((always_inline)) {
#pragma unroll
    for (int k = 0; k < NPRE; ++k) {
      const int e = tid + 256 * k;
      if (e >= SLOTS) continue;
      const int r = e / KS, c = e - r * KS;
      v4 v = pre[k];                                                       // (the padding is zeroed here, not at the load: a select on
      if (d != 4 * KS) {                                                   //  the loaded value would wait for it before the MFMAs)
#pragma unroll
        for (int q = 0; q < 4; ++q) v[q] = 4 * c + q < d ? v[q] : 0.f;
      }
      Xb[buf * STG + r * ROW4 + c] = v;
    }
    if (tid < ST) Xb[buf * STG + tid * ROW4 + KS] = (v4){pre_add, 0.f, 0.f, 0.f};
  };
  // ---- ranking (see ktup_eval_pass.hip): candidates are appended to the user's pending row in LDS at positions taken from a ballot
  // (`pend` is replicated over the row's 16 lanes); once a row of a register slot holds 16, that slot's four rows go through the
  // merge network and the n-th keys are renewed
  const int rowbase = 16 * kq;
  const RowAppend app(kq, j);
  auto flush = [&](bool all) __attribute__((always_inline)) {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
#pragma unroll
    for (int reg = 0; reg < 4; ++reg) {
      const int n = pend[reg];
      if (!__builtin_amdgcn_ballot_w64(all ? n > 0 : n >= 16)) continue;
      const int ur = 4 * kq + reg;
      const uint64_t* row = pbuf + ur * PCAP;
      const uint64_t merged = row_merge_pending(tk[ur * 16 + j], row, n, topn, j);   // all four rows of the slot at once
      tk[ur * 16 + j] = merged;
      pend[reg] = 0;
      const uint32_t nhi = (uint32_t)__shfl((int)(uint32_t)(merged >> 32), rowbase + topn - 1, 64);
      const uint32_t nlo = (uint32_t)__shfl((int)(uint32_t)merged, rowbase + topn - 1, 64);
      if (u0 + ur < a.nq) {                                                           // (rows past the end keep 0 / +inf)
        thr[reg] = ((uint64_t)nhi << 32) | nlo;
        thrf[reg] = -topn_key_score(nhi);                                               // negated back (NaN: list short)
      }
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
  };
  auto rank_tile = [&](const v4& acc, float iadd, int64_t item) __attribute__((always_inline)) {         // 16 users x the 16 items [item - j, item - j + 16)
    const bool iok = item < i_hi;
    bool full = false;
#pragma unroll
    for (int reg = 0; reg < 4; ++reg) {
      const int ur = 4 * kq + reg;
      float s = acc[reg];
      if (a.user_add) s = __fadd_rn(s, uadd[reg]);
      if (a.item_add) s = __fadd_rn(s, iadd);
      const bool above = s > thrf[reg], maybe = !(s < thrf[reg]) && iok;
      if (!__builtin_amdgcn_ballot_w64(maybe)) continue;                   // most 64-score slots leave here
      const uint64_t key = topn_key(s, true, (uint32_t)item);
      bool c = maybe && (above || key < thr[reg]);
      if (c && a.bm) c = ((a.bm[(u0 + ur) * a.bm_words + (item >> 5)] >> (item & 31)) & 1u) == 0u;
      const uint64_t m = __builtin_amdgcn_ballot_w64(c);
      if (m) {
        app.put(pbuf, ur * PCAP, pend[reg], m, c, [&] { return key; });
        full |= pend[reg] >= 16;
      }
    }
    if (__builtin_amdgcn_ballot_w64(full)) flush(false);
  };
  auto compute = [&](int buf, int64_t row0) __attribute__((always_inline)) {
    const float* rb = reinterpret_cast<const float*>(Xb + buf * STG + j * ROW4) + kq;   // lane (kq, item j): element kq of every k quad
    v4 acc[NSUB];
#pragma unroll
    for (int t = 0; t < NSUB; ++t) acc[t] = (v4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int s = 0; s < KS; ++s) {
#pragma unroll
      for (int t = 0; t < NSUB; ++t) acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[s], rb[t * 16 * ROW4 * 4 + 4 * s], acc[t], 0, 0, 0);
    }
#pragma unroll
    for (int t = 0; t < NSUB; ++t) {
      if (row0 + 16 * t >= i_hi) break;                                    // (uniform)
      rank_tile(acc[t], rb[t * 16 * ROW4 * 4 + 4 * KS - kq], row0 + 16 * t + j);
    }
  };
  const int64_t nst = (i_hi - i_lo + ST - 1) / ST;
  fetch(i_lo);
  stash(0);
  __syncthreads();                                                         // stage 0 and the lists are in place
  // one stage per workgroup barrier; the next stage's loads are in flight under this stage's MFMAs.  Buffer buf ^ 1 was last read in
  // the previous iteration, whose closing barrier every wave has passed; its new contents are read after this iteration's barrier.
  for (int64_t t0 = 0; t0 < nst; ++t0) {
    const int buf = (int)(t0 & 1);
    const bool more = t0 + 1 < nst;
    if (more) fetch(i_lo + (t0 + 1) * ST);
    __builtin_amdgcn_sched_barrier(0);                                     // the loads are issued before, their values used after the MFMAs
    compute(buf, i_lo + t0 * ST);
    __builtin_amdgcn_sched_barrier(0);
    if (more) stash(buf ^ 1);
    __syncthreads();
  }
  flush(true);
  if (j < topn) {
#pragma unroll
    for (int reg = 0; reg < 4; ++reg) {
      const int64_t ur = u0 + 4 * kq + reg;
      if (ur < a.nq) a.part[(ur * a.nsplit + sp) * topn + j] = tk[(4 * kq + reg) * 16 + j];
    }
  }
}

template <int KS>
int launch_dot_pass(const DotArgs& a, unsigned blocks, hipStream_t st, const char* name) {
  const size_t lds = DotGeom<KS>::LDS;
  static_assert(DotGeom<KS>::LDS <= 160 * 1024, "the stages and the lists fit the LDS");
  if (a.ivec) {
    (void)hipFuncSetAttribute((const void*)dot_pass_kernel<KS, true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    hipLaunchKernelGGL((dot_pass_kernel<KS, true>), dim3(blocks), dim3(256), lds, st, a);
  } else {
    (void)hipFuncSetAttribute((const void*)dot_pass_kernel<KS, false>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    hipLaunchKernelGGL((dot_pass_kernel<KS, false>), dim3(blocks), dim3(256), lds, st, a);
  }
  return check_launch(name);
}

// how the catalogue is cut: `want` splits, whole 16-item tiles each.  0: about 1.25 workgroups per CU.  Every split keeps a list of
// its own per user, so more splits mean more candidates through the append / merge path and a prologue each; fewer leave CUs idle.
// Measured (one MI355X, d = 64, topn 10, ~165 filtered ids per user, whole call): 6040 x 3240: 4 splits 143 us (1: 260, 8: 165,
// 12: 189); 512 x 100,000: 32 splits 279 us (16: 431, 8: 710); 30,000 x 25,000: 1 split 1.76 ms (3: 2.09, 8: 2.50).
int dot_nsplit(int64_t nq, int64_t n_items, int want, int64_t* split_items) {
  const int64_t nub = (nq + 63) / 64;
  int64_t ns = want > 0 ? want : (320 + nub - 1) / (nub > 0 ? nub : 1);
  ns = ns < 1 ? 1 : ns > NSPLIT_MAX ? NSPLIT_MAX : ns;
  int64_t si = (n_items + ns - 1) / ns;
  si = (si + 15) / 16 * 16;
  if (want <= 0 && si < 256) si = 256;                                     // (a workgroup's prologue wants some items to pay for it)
  *split_items = si;
  return (int)((n_items + si - 1) / si);
}

}  // namespace
}  // namespace ktup

using namespace ktup;

extern "C" size_t ktup_eval_dot_topk_workspace_bytes(int d, int64_t nq, int64_t n_items, int topn, int nsplit) {
  (void)d;
  if (nq <= 0 || n_items <= 0 || topn <= 0 || topn > TOPN_MAX || nsplit < 0) return 0;
  int64_t si = 0;
  const int ns = dot_nsplit(nq, n_items, nsplit, &si);
  const size_t part = (size_t)nq * ns * topn * sizeof(uint64_t);
  const size_t bits = (size_t)nq * (size_t)((n_items + 31) / 32) * sizeof(uint32_t);
  return part + bits + 16;
}

extern "C" int ktup_eval_dot_topk(const float* U, int64_t ldu, const float* I, int64_t ldi, int d, const int64_t* u_ids, int64_t nq,
                                  int64_t n_items, const float* user_add, const float* item_add, const int64_t* filt_off,
                                  const int32_t* filt_ids, int topn, int nsplit, int32_t* top_ids, float* top_scores, void* ws,
                                  void* stream) {
  const char* name = "ktup_eval_dot_topk";
  KTUP_REQUIRE(U && I && u_ids && top_ids && ws, "%s: null table, id, output or workspace pointer", name);
  KTUP_REQUIRE(d >= 1 && nq >= 0 && n_items > 0 && topn > 0 && nsplit >= 0, "%s: bad sizes (embedding_size %d, %lld users, %lld items, topn %d, nsplit %d)",
               name, d, (long long)nq, (long long)n_items, topn, nsplit);
  KTUP_REQUIRE(ldu >= d && ldi >= d, "%s: a row pitch is below embedding_size %d", name, d);
  KTUP_REQUIRE((filt_off == nullptr) == (filt_ids == nullptr), "%s: filt_off and filt_ids go together", name);
  KTUP_REQUIRE((reinterpret_cast<uintptr_t>(ws) & 15) == 0, "%s: the workspace must be 16-byte aligned", name);
  if (topn > TOPN_MAX) return set_error(KTUP_ERR_UNSUPPORTED, "%s: topn %d > %d", name, topn, TOPN_MAX);
  if (d > 256) return set_error(KTUP_ERR_UNSUPPORTED, "%s: embedding_size %d > 256", name, d);
  if (n_items >= ((int64_t)1 << 31)) return set_error(KTUP_ERR_UNSUPPORTED, "%s: %lld items do not fit 32-bit ids", name, (long long)n_items);
  if (nq == 0) return KTUP_OK;
  hipStream_t st = (hipStream_t)stream;
  DotArgs a;
  a.U = U; a.ldu = ldu; a.I = I; a.ldi = ldi; a.d = d;
  a.ivec = (d % 4 == 0 && ldi % 4 == 0 && (reinterpret_cast<uintptr_t>(I) & 15) == 0) ? 1 : 0;
  a.u_ids = u_ids; a.nq = nq; a.n_items = n_items; a.user_add = user_add; a.item_add = item_add;
  a.topn = topn;
  a.nsplit = dot_nsplit(nq, n_items, nsplit, &a.split_items);
  a.part = reinterpret_cast<uint64_t*>(ws);
  a.bm = nullptr;
  a.bm_words = (n_items + 31) / 32;
  const int64_t nub = (nq + 63) / 64;
  if (nub * a.nsplit > 0x7fffffffLL) return set_error(KTUP_ERR_UNSUPPORTED, "%s: too many users for one call (%lld)", name, (long long)nq);
  if (filt_off) {
    // (after the partial lists: 8-byte entries, so the bits start on an 8-byte boundary)
    uint32_t* bm = reinterpret_cast<uint32_t*>(a.part + (size_t)nq * a.nsplit * topn);
    const int64_t nw = nq * a.bm_words;
    hipLaunchKernelGGL(dot_filter_zero_kernel, dim3((unsigned)min((nw + 255) / 256, (int64_t)4096)), dim3(256), 0, st, bm, nw);
    if (int rc = check_launch(name)) return rc;
    hipLaunchKernelGGL(dot_filter_bits_kernel, dim3((unsigned)min((nq + 3) / 4, (int64_t)4096)), dim3(256), 0, st, filt_off, filt_ids, nq, n_items,
                       bm, a.bm_words);
    if (int rc = check_launch(name)) return rc;
    a.bm = bm;
  }
  const unsigned blocks = (unsigned)(nub * a.nsplit);
  const int nk = (d + 3) / 4;
  int rc;
  if (nk <= 5) rc = launch_dot_pass<5>(a, blocks, st, name);
  else if (nk <= 9) rc = launch_dot_pass<9>(a, blocks, st, name);
  else if (nk <= 16) rc = launch_dot_pass<16>(a, blocks, st, name);
  else if (nk <= 25) rc = launch_dot_pass<25>(a, blocks, st, name);
  else if (nk <= 32) rc = launch_dot_pass<32>(a, blocks, st, name);
  else if (nk <= 48) rc = launch_dot_pass<48>(a, blocks, st, name);
  else rc = launch_dot_pass<64>(a, blocks, st, name);
  if (rc) return rc;
  hipLaunchKernelGGL((topk_merge_kernel<MERGE_PER_LANE, true>), dim3((unsigned)((nq + 3) / 4)), dim3(MERGE_T), 0, st, a.part, nq, a.nsplit, topn, top_ids,
                     top_scores);
  return check_launch(name);
}
