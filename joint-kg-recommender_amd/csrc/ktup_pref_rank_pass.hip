// The filtered rank of EVERY gold item of a TUP / KTUP evaluation pass (soft gate, squared L2) in one sweep that never writes the
// (users x items) matrix: ktup_eval_pref_ranks -- what ktup_eval_gold_ranks(descending = 0) returns on the scores of
// ktup_eval_pref_topk, the rank form of the preference-space list pass (ktup_eval_pass.hip eval_pass_q_kernel) as
// ktup_eval_dot_ranks / ktup_eval_cfkg_ranks (ktup_rank_pass.hip) are the rank forms of the inner-product and CFKG list passes.
//
// A rank is a COUNT: rank(g) = #{items of the user ordered before g that are neither filtered nor gold}, the order being the list
// pass's 64-bit key topn_key(score, false, id): ascending score, ties -> lower id.  The scores are the list pass's BITS: the operand
// tables A / SCU / B come from the list pass's own host function (pref_q_tables: the same Gram and row kernels by the same rule), and
// the A-operand load, the 16-item LDS-DMA tiles, the MFMA chain and the four-term epilogue are the one copy in ktup_pref_q_tile.h.
// Two launches after the tables and the per-pass filter bitmap (sweep_filter_bits, [nq][ceil(n / 32)]):
//   * pref_rank_keys_kernel, one workgroup per 64 users: the block's concatenated gold ids stream through the tiles AS the candidate
//     list -- every LDS-DMA slot takes its source from B + gold_id * GROW (an id outside the catalogue reads row 0 and gets "no key")
//     -- and lane (user, entry) keeps the key where the entry lies in that user's own range; a filtered gold gets PKEY_MAX.  A wave
//     runs the chain only on the tiles that hold entries of its 16 users.  The keys are sorted per user by counting; keys,
//     permutation and the initial ranks (0 / -1) go to the workspace;
//   * pref_rank_count_kernel, one workgroup per (64 users, catalogue split), PLAIN mapping (user block major: blockIdx.x = block x
//     nsplit + split; the list pass's XCD-aware mapping exists for its shared per-user bounds, which this pass does not have): user
//     operands in registers, item tiles double-buffered by LDS-DMA exactly as in the list pass; in place of pending rows and lists the
//     LDS holds the block's sorted gold keys and one 32-bit counter per gold slot.  A score that is not below or equal to the user's
//     worst gold score leaves after one float compare and one ballot; a survivor builds its key, reads its filter bit from the
//     bitmap in global memory, binary-searches the user's keys, skips an equal key (the gold itself) and bumps the bucket with an LDS
//     integer add.  The prefix sums over a user's buckets are added to `ranks` with integer global atomics: exact in any order, so a
//     rank is the same integer at every nsplit.  No float atomics, no scratch.
// LDS: two tiles + four waves' user scalars + the block's offsets + 12 bytes per gold entry; PREF_RANK_LDS_MAX below fixes the cap.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <type_traits>

#include "ktup_common.h"
#include "ktup_lane_swap.h"
#include "ktup_pref_geom.h"
#include "ktup_pref_q_tile.h"
#include "ktup_sweep_pass.h"
#include "ktup_topn.h"

namespace ktup {
namespace {

constexpr size_t PR_USC_BYTES = (size_t)4 * 16 * 4 * sizeof(float);     // four waves' user scalars [16][4]
constexpr size_t PR_OFF_BYTES = 80 * sizeof(int);                       // the block's 65 offsets
template <typename G>
constexpr size_t pr_fixed_lds() { return (size_t)2 * G::TILE_F4 * 16 + PR_USC_BYTES + PR_OFF_BYTES; }
// ... | gcap sorted keys | gcap counters
template <typename G>
constexpr size_t pr_lds(int64_t gcap) { return pr_fixed_lds<G>() + (size_t)gcap * (sizeof(uint64_t) + sizeof(uint32_t)); }
// Two workgroups per CU at every covered geometry with the full cap (include/ktup_hip.h KTUP_PREF_RANK_BLOCK_GOLDS): the worst case,
// d = 128 with 21 - 32 preferences, is 2 x 916 float4 of tiles (29,312 B) + 1,024 + 320 + 12 x 3072 (36,864 B) = 67,520 B of 81,920
constexpr size_t PREF_RANK_LDS_MAX = 160 * 1024 / 2;
static_assert(pr_lds<QGeom<32, 8>>(KTUP_PREF_RANK_BLOCK_GOLDS) <= PREF_RANK_LDS_MAX && pr_lds<QGeom<32, 5>>(KTUP_PREF_RANK_BLOCK_GOLDS) <= PREF_RANK_LDS_MAX &&
                  pr_lds<QGeom<25, 8>>(KTUP_PREF_RANK_BLOCK_GOLDS) <= PREF_RANK_LDS_MAX && pr_lds<QGeom<16, 8>>(KTUP_PREF_RANK_BLOCK_GOLDS) <= PREF_RANK_LDS_MAX,
              "two tiles, the user scalars, the offsets and 12 bytes per gold entry fit the LDS twice per CU");

struct PrefRankArgs {
  const float *A, *SCU;                 // users: AROW floats + 4 scalars each
  const float* B;                       // items: rows of GROW floats (operands, then the 4 scalars)
  int64_t nq, n;                        // users and items of the pass
  const uint32_t* bm; int64_t bm_words; // the filter bits [nq][bm_words]; NULL = no filter
  const int64_t* gold_off; const int32_t* gold_ids;
  uint64_t* skey;                       // [n_gold] every user's gold keys, ascending ("no key" last)
  int32_t* perm;                        // [n_gold] which entry of the block (relative to its first) the sorted slot holds
  int32_t* ranks;
  int gcap;                             // gold entries per block the launch's LDS holds (a multiple of 64)
  int nsplit; int64_t split;            // items per split (whole 16-item tiles)
};

// what both kernels find in their LDS after the two tiles
template <typename G>
struct PrLds {
  v4* Xb; float* usc; int* goff; uint64_t* gk; uint32_t* cnt;
  KTUP_DEV PrLds(char* smem, int w, int gcap) {
    Xb = reinterpret_cast<v4*>(smem);                                     // [2][TILE_F4] item tiles
    char* p = smem + (size_t)2 * G::TILE_F4 * 16;
    usc = reinterpret_cast<float*>(p) + w * 64;                           // this wave's [16][4] user scalars
    goff = reinterpret_cast<int*>(p + PR_USC_BYTES);
    gk = reinterpret_cast<uint64_t*>(p + PR_USC_BYTES + PR_OFF_BYTES);
    cnt = reinterpret_cast<uint32_t*>(gk + gcap);
  }
};

// the block's gold range and, in LDS, its users' offsets relative to it (users past the end: empty ranges at the end)
struct PrBlock { int64_t g_lo; int64_t ng; };
KTUP_DEV PrBlock pr_block(const PrefRankArgs& a, int64_t ub, int* goff) {
  const int64_t b0 = ub * 64;
  const int64_t g_lo = a.gold_off[b0];
  const int64_t ng = a.gold_off[min(a.nq, b0 + 64)] - g_lo;
  if (ng > 0 && ng <= a.gcap && threadIdx.x <= 64) goff[threadIdx.x] = (int)(a.gold_off[min(a.nq, b0 + (int64_t)threadIdx.x)] - g_lo);
  return PrBlock{g_lo, ng};
}

template <typename G>
__global__ __launch_bounds__(256, 2) void pref_rank_keys_kernel(PrefRankArgs a) {
  constexpr int RB4 = G::RB4, ROW4 = G::ROW4;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x, lane = tid & 63, kq = lane >> 4, j = lane & 15;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const PrLds<G> L(smem, w, a.gcap);
  v4* Xb = L.Xb;
  const int64_t ub = blockIdx.x;
  const PrBlock blk = pr_block(a, ub, L.goff);
  if (blk.ng <= 0) return;                                                 // (uniform exits: before every barrier)
  if (blk.ng > a.gcap) {                                                   // more than the caller announced: nothing of the block is ranked
    for (int64_t e = tid; e < blk.ng; e += 256) a.ranks[blk.g_lo + e] = -1;
    return;
  }
  const int64_t g_lo = blk.g_lo;
  const int ng = (int)blk.ng;
  const int64_t u0 = ub * 64 + 16 * w;
  for (int idx = tid; idx < 2 * G::TILE_F4; idx += 256) Xb[idx] = (v4){0.f, 0.f, 0.f, 0.f};   // row pads stay finite (x 0 operands)
  if (lane < 16) *reinterpret_cast<v4*>(L.usc + lane * 4) =
      u0 + lane < a.nq ? *reinterpret_cast<const v4*>(a.SCU + (u0 + lane) * 4) : (v4){0.f, 0.f, 0.f, 0.f};
  KTUP_Q_USER_OPS(G, u0 + j < a.nq, a.A + (ok ? u0 + j : 0) * G::AROW, kq)
  __syncthreads();                                                         // tiles zeroed, offsets and scalars in place
  int lo[4], hi[4];
#pragma unroll
  for (int reg = 0; reg < 4; ++reg) {
    lo[reg] = L.goff[16 * w + 4 * kq + reg];
    hi[reg] = L.goff[16 * w + 4 * kq + reg + 1];
  }
  const int wlo = L.goff[16 * w], whi = L.goff[16 * w + 16];               // the entries of this wave's users
  KTUP_Q_DMA_OFFSETS(G, soff, w, lane)
  // tile t = entries 16 t .. 16 t + 15 of the block: slot (row, c) from row gold_ids[entry] of B, the address arithmetic of the list
  // pass's tail tiles per row (an entry past the end or an id outside the catalogue: row 0, finite operands nobody keeps)
  auto dma = [&](int t, int buf) {
    v4* dst = Xb + buf * G::TILE_F4 + 64 * w;
#pragma unroll
    for (int k = 0; k < G::DPW; ++k) {
      if (soff[k] == 0xffffffffu) continue;
      const uint32_t slot = soff[k] >> 4, row = slot / ROW4, c = slot - row * ROW4;
      const int e = 16 * t + (int)row;
      int64_t id = e < ng ? (int64_t)a.gold_ids[g_lo + e] : 0;
      if (id < 0 || id >= a.n) id = 0;
      const char* from = reinterpret_cast<const char*>(a.B + id * G::GROW + 4 * c);
      __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)from,
                                       (__attribute__((address_space(3))) void*)(dst + 256 * k), 16, 0, 0);
    }
  };
  auto compute = [&](int buf, int t) {                                     // 16 users x the 16 entries of tile t
    KTUP_Q_TILE_MFMA(G, Xb + buf * G::TILE_F4 + j * ROW4, kq)               // lane (kq, entry j) -> accAA, accS, accAN, accNN
    const v4 is4 = Xb[buf * G::TILE_F4 + j * ROW4 + RB4];                  // the row's scalars ride in its tile slot
    const int e = 16 * t + j;
    const bool eok = e < ng;
    const int64_t id = a.gold_ids[g_lo + (eok ? e : ng - 1)];
    const bool ranked = id >= 0 && id < a.n;
#pragma unroll
    for (int reg = 0; reg < 4; ++reg) {
      if (!(eok && e >= lo[reg] && e < hi[reg])) continue;                 // the entry is this user's own
      const int ur = 4 * kq + reg;
      const v4 us4 = *reinterpret_cast<const v4*>(L.usc + ur * 4);
      const float score = q_score(us4, is4, accS[reg], accAA[reg], accAN[reg], accNN[reg]);
      bool v = ranked;
      if (v && a.bm) v = ((a.bm[(u0 + ur) * a.bm_words + (id >> 5)] >> (id & 31)) & 1u) == 0u;
      L.gk[e] = v ? topn_key(score, false, (uint32_t)id) : PKEY_MAX;
    }
  };
  const int ntile = (ng + IBT - 1) / IBT;
  dma(0, 0);
  __syncthreads();                                                         // (carries the vmcnt(0) that lands the DMA)
  for (int t0 = 0; t0 < ntile; ++t0) {
    const int buf = t0 & 1;
    if (t0 + 1 < ntile) dma(t0 + 1, buf ^ 1);
    if (16 * t0 < whi && 16 * t0 + 16 > wlo) compute(buf, t0);             // (wave-uniform: the other waves' users own this tile)
    __syncthreads();
  }
  // (the last barrier is behind every wave: all keys are in place)  A wave sorts its 16 users' keys by counting: equal keys -- an id
  // that occurs twice -- stay in entry order
  for (int ur = 16 * w; ur < 16 * w + 16; ++ur) {
    const int l0 = L.goff[ur], l1 = L.goff[ur + 1];
    for (int i = l0 + lane; i < l1; i += 64) {
      const uint64_t k = L.gk[i];
      int pos = 0;
      for (int o = l0; o < l1; ++o) {
        const uint64_t ko = L.gk[o];
        pos += (ko < k || (ko == k && o < i)) ? 1 : 0;
      }
      a.skey[g_lo + l0 + pos] = k;
      a.perm[g_lo + l0 + pos] = i;
      a.ranks[g_lo + i] = k == PKEY_MAX ? -1 : 0;
    }
  }
}

template <typename G>
__global__ __launch_bounds__(256, 2) void pref_rank_count_kernel(PrefRankArgs a) {
  constexpr int RB4 = G::RB4, ROW4 = G::ROW4;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x, lane = tid & 63, kq = lane >> 4, j = lane & 15;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const PrLds<G> L(smem, w, a.gcap);
  v4* Xb = L.Xb;
  const int64_t ub = (int64_t)(blockIdx.x / (unsigned)a.nsplit);
  const int sp = (int)(blockIdx.x - (unsigned)ub * (unsigned)a.nsplit);
  const PrBlock blk = pr_block(a, ub, L.goff);
  if (blk.ng <= 0 || blk.ng > a.gcap) return;                              // (uniform: before every barrier)
  const int64_t g_lo = blk.g_lo;
  for (int i = tid; i < (int)blk.ng; i += 256) {
    L.gk[i] = a.skey[g_lo + i];
    L.cnt[i] = 0u;
  }
  const int64_t u0 = ub * 64 + 16 * w;
  const int64_t i_lo = (int64_t)sp * a.split;
  const int64_t i_hi = min(a.n, i_lo + a.split);
  for (int idx = tid; idx < 2 * G::TILE_F4; idx += 256) Xb[idx] = (v4){0.f, 0.f, 0.f, 0.f};   // row pads stay finite (x 0 operands)
  if (lane < 16) *reinterpret_cast<v4*>(L.usc + lane * 4) =
      u0 + lane < a.nq ? *reinterpret_cast<const v4*>(a.SCU + (u0 + lane) * 4) : (v4){0.f, 0.f, 0.f, 0.f};
  KTUP_Q_USER_OPS(G, u0 + j < a.nq, a.A + (ok ? u0 + j : 0) * G::AROW, kq)
  __syncthreads();                                                         // tiles zeroed; keys, counters, offsets and scalars in place
  // per accumulator row: where the user's keys start, how many are real, the worst of them and its score (no real key: nothing is
  // ever ordered before -- key 0 / -inf, as the list pass's rows past the end)
  int lo[4], nv[4];
  uint64_t thr[4];
  float thrf[4];
#pragma unroll
  for (int reg = 0; reg < 4; ++reg) {
    const int ur = 16 * w + 4 * kq + reg;
    lo[reg] = L.goff[ur];
    int l = 0, h = L.goff[ur + 1] - lo[reg];
    while (l < h) {
      const int m = (l + h) >> 1;
      if (L.gk[lo[reg] + m] != PKEY_MAX) l = m + 1; else h = m;
    }
    nv[reg] = l;
    thr[reg] = l > 0 ? L.gk[lo[reg] + l - 1] : 0ull;
    thrf[reg] = l > 0 ? topn_key_score((uint32_t)(thr[reg] >> 32)) : -__builtin_inff();
  }
  KTUP_Q_DMA_OFFSETS(G, soff, w, lane)
  auto dma = [&](int64_t t, int buf) {                                     // tile t of this split -> LDS buffer `buf`
    KTUP_Q_TILE_DMA(G, a.B, a.n, i_lo + t * IBT, Xb + buf * G::TILE_F4 + 64 * w, soff)
  };
  auto compute = [&](int buf, int64_t t) {                                 // 16 users x the 16 items of tile t
    KTUP_Q_TILE_MFMA(G, Xb + buf * G::TILE_F4 + j * ROW4, kq)               // lane (kq, item j) -> accAA, accS, accAN, accNN
    const v4 is4 = Xb[buf * G::TILE_F4 + j * ROW4 + RB4];                  // the row's scalars ride in its tile slot
    const int64_t item = i_lo + t * IBT + j;
    const bool iok = item < i_hi;
#pragma unroll
    for (int reg = 0; reg < 4; ++reg) {
      const int ur = 4 * kq + reg;
      const v4 us4 = *reinterpret_cast<const v4*>(L.usc + ur * 4);
      const float score = q_score(us4, is4, accS[reg], accAA[reg], accAN[reg], accNN[reg]);
      const bool below = score < thrf[reg], maybe = !(score > thrf[reg]) && iok;      // (unordered: the keys decide)
      if (!__builtin_amdgcn_ballot_w64(maybe)) continue;                   // most 64-score slots leave here
      const uint64_t key = topn_key(score, false, (uint32_t)item);
      bool c = maybe && (below || key < thr[reg]) && nv[reg] > 0;
      if (c && a.bm) c = ((a.bm[(u0 + ur) * a.bm_words + (item >> 5)] >> (item & 31)) & 1u) == 0u;
      if (c) {
        const uint64_t* keys = L.gk + lo[reg];
        int l = 0, h = nv[reg] - 1;                                        // the first gold key that is not before this one (the worst is not)
        while (l < h) {
          const int m = (l + h) >> 1;
          if (keys[m] < key) l = m + 1; else h = m;
        }
        if (keys[l] != key) atomicAdd(L.cnt + lo[reg] + l, 1u);            // (the same key is the same item: the gold itself)
      }
    }
  };
  const int64_t ntile = (i_hi - i_lo + IBT - 1) / IBT;
  if (ntile > 0) {
    dma(0, 0);
    __syncthreads();                                                       // (carries the vmcnt(0) that lands the DMA)
  }
  // one tile per workgroup barrier; the next tile's DMA is in flight under this tile's MFMAs, as in the list pass
  for (int64_t t0 = 0; t0 < ntile; ++t0) {
    const int buf = (int)(t0 & 1);
    if (t0 + 1 < ntile) dma(t0 + 1, buf ^ 1);
    compute(buf, t0);
    __syncthreads();
  }
  // (behind the last barrier)  One thread per user: the running sum over its buckets is the split's share of each rank
  if (tid < 64) {
    const int l0 = L.goff[tid], l1 = L.goff[tid + 1];
    uint32_t run = 0u;
    for (int p = l0; p < l1; ++p) {
      if (L.gk[p] == PKEY_MAX) break;
      run += L.cnt[p];
      if (run) atomicAdd(a.ranks + g_lo + a.perm[g_lo + p], (int32_t)run);
    }
  }
}

template <typename G>
int launch_pref_rank(const PrefRankArgs& a, hipStream_t st, const char* name) {
  const size_t lds = pr_lds<G>(a.gcap);
  const unsigned nub = (unsigned)((a.nq + 63) / 64);
  (void)hipFuncSetAttribute((const void*)pref_rank_keys_kernel<G>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  (void)hipFuncSetAttribute((const void*)pref_rank_count_kernel<G>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  hipLaunchKernelGGL((pref_rank_keys_kernel<G>), dim3(nub), dim3(256), lds, st, a);
  if (int rc = check_launch(name)) return rc;
  hipLaunchKernelGGL((pref_rank_count_kernel<G>), dim3(nub * (unsigned)a.nsplit), dim3(256), lds, st, a);
  return check_launch(name);
}

template <int NCH>
int launch_pref_rank_p(int n_pref, const PrefRankArgs& a, hipStream_t st, const char* name) {
  if (n_pref <= 4) return launch_pref_rank<QGeom<NCH, 1>>(a, st, name);
  if (n_pref <= 20) return launch_pref_rank<QGeom<NCH, 5>>(a, st, name);
  return launch_pref_rank<QGeom<NCH, 8>>(a, st, name);
}

// the shapes the pass serves: soft gate with squared L2 at the list pass's narrow widths, on the matrix cores
bool pref_rank_shape_ok(int d, int n_pref, int l1, int64_t n, int64_t block_golds) {
  return !l1 && (d == 64 || d == 100 || d == 128) && n_pref >= 1 && n_pref <= 32 && opt_eval_mc() && n > 0 && n < ((int64_t)1 << 31) &&
         block_golds >= 0 && block_golds <= KTUP_PREF_RANK_BLOCK_GOLDS;
}

// workspace: the sorted keys (8-byte entries) | their permutation (padded to 8 bytes) | the filter bits (padded to 16 bytes) | the
// operand tables (pref_q_tables_bytes)
size_t pr_perm_bytes(int64_t n_gold) { return ((size_t)n_gold * sizeof(int32_t) + 7) / 8 * 8; }
size_t pr_bits_bytes(int64_t nq, int64_t n) { return ((size_t)nq * (size_t)((n + 31) / 32) * sizeof(uint32_t) + 15) / 16 * 16; }

}  // namespace
}  // namespace ktup

using namespace ktup;

extern "C" int ktup_eval_pref_ranks_supported(int d, int n_pref, int l1, int64_t n_items, int64_t block_golds) {
  return pref_rank_shape_ok(d, n_pref, l1, n_items, block_golds) ? 1 : 0;
}

extern "C" size_t ktup_eval_pref_ranks_workspace_bytes(int d, int n_pref, int l1, int64_t nq, int64_t n_items, int64_t n_gold, int64_t block_golds) {
  if (nq <= 0 || n_gold <= 0 || !pref_rank_shape_ok(d, n_pref, l1, n_items, block_golds)) return 0;
  return (size_t)n_gold * sizeof(uint64_t) + pr_perm_bytes(n_gold) + pr_bits_bytes(nq, n_items) + pref_q_tables_bytes(d, n_pref, nq, n_items) + 16;
}

extern "C" int ktup_eval_pref_ranks(const float* U, int64_t ldu, const float* I, int64_t ldi, const float* E, int64_t lde, const int32_t* item2ent,
                                    const float* pref_ws, int n_pref, int d, const int64_t* u_ids, int64_t nq, int64_t n_items, int l1,
                                    const int64_t* filt_off, const int32_t* filt_ids, const int64_t* gold_off, const int32_t* gold_ids,
                                    int64_t n_gold, int64_t block_golds, int nsplit, int32_t* ranks, void* ws, void* stream) {
  const char* name = "ktup_eval_pref_ranks";
  KTUP_REQUIRE(U && I && pref_ws, "%s: null table pointer", name);
  KTUP_REQUIRE((E == nullptr) == (item2ent == nullptr), "%s: E and item2ent must be given together", name);
  KTUP_REQUIRE(d >= 1 && n_pref >= 1 && n_items > 0, "%s: bad sizes (embedding_size %d, %d preferences, %lld items)", name, d, n_pref, (long long)n_items);
  KTUP_REQUIRE(ldu >= d && ldi >= d && (!E || lde >= d), "%s: a row pitch is below embedding_size %d", name, d);
  KTUP_REQUIRE(nq >= 0 && n_gold >= 0 && nsplit >= 0 && block_golds >= 0, "%s: bad sizes (%lld users, n_gold %lld, block_golds %lld, nsplit %d)", name,
               (long long)nq, (long long)n_gold, (long long)block_golds, nsplit);
  KTUP_REQUIRE((filt_off == nullptr) == (filt_ids == nullptr), "%s: filt_off and filt_ids go together", name);
  KTUP_REQUIRE(gold_off, "%s: null gold_off", name);
  KTUP_REQUIRE(gold_ids || n_gold == 0, "%s: gold_off without gold_ids (n_gold %lld)", name, (long long)n_gold);
  KTUP_REQUIRE(ranks || n_gold == 0, "%s: null ranks", name);
  KTUP_REQUIRE(block_golds <= n_gold, "%s: block_golds %lld above n_gold %lld", name, (long long)block_golds, (long long)n_gold);
  if (l1) return set_error(KTUP_ERR_UNSUPPORTED, "%s: the squared-L2 soft gate only (L1 keeps the matrix route)", name);
  if (d != 64 && d != 100 && d != 128) return set_error(KTUP_ERR_UNSUPPORTED, "%s: embedding_size %d is not one of 64, 100, 128", name, d);
  if (n_pref > 32) return set_error(KTUP_ERR_UNSUPPORTED, "%s: %d preferences > 32", name, n_pref);
  if (!opt_eval_mc()) return set_error(KTUP_ERR_UNSUPPORTED, "%s: option eval_mc is 0", name);
  if (n_items >= ((int64_t)1 << 31)) return set_error(KTUP_ERR_UNSUPPORTED, "%s: %lld items do not fit 32-bit ids", name, (long long)n_items);
  if (block_golds > KTUP_PREF_RANK_BLOCK_GOLDS)
    return set_error(KTUP_ERR_UNSUPPORTED, "%s: a 64-user block with %lld gold entries (at most %d)", name, (long long)block_golds,
                     KTUP_PREF_RANK_BLOCK_GOLDS);
  if (nq == 0 || n_gold == 0) return KTUP_OK;
  KTUP_REQUIRE(u_ids && ws, "%s: null id or workspace pointer", name);
  KTUP_REQUIRE((reinterpret_cast<uintptr_t>(ws) & 15) == 0, "%s: the workspace must be 16-byte aligned", name);
  KTUP_REQUIRE(aligned16(pref_ws), "%s: the preference workspace must be 16-byte aligned", name);
  const PrefGeom g = pref_geom(d, n_pref);
  hipStream_t st = (hipStream_t)stream;
  PrefRankArgs a{};
  a.nq = nq; a.n = n_items; a.gold_off = gold_off; a.gold_ids = gold_ids; a.ranks = ranks;
  a.gcap = (int)((block_golds + 63) / 64 * 64);
  if (a.gcap < 64) a.gcap = 64;
  a.nsplit = sweep_nsplit(nq, n_items, TOPN_MAX, nsplit, &a.split);
  if ((nq + 63) / 64 * a.nsplit > 0x7fffffffLL) return set_error(KTUP_ERR_UNSUPPORTED, "%s: too many users for one call (%lld)", name, (long long)nq);
  a.skey = reinterpret_cast<uint64_t*>(ws);
  a.perm = reinterpret_cast<int32_t*>(a.skey + n_gold);
  uint32_t* bm = reinterpret_cast<uint32_t*>(reinterpret_cast<char*>(a.perm) + pr_perm_bytes(n_gold));
  char* tables = reinterpret_cast<char*>(bm) + pr_bits_bytes(nq, n_items);
  tables += (16 - (reinterpret_cast<uintptr_t>(tables) & 15)) & 15;
  a.bm = nullptr;
  a.bm_words = (n_items + 31) / 32;
  PrefQTables t{};
  if (int rc = pref_q_tables(U, ldu, u_ids, nq, I, ldi, E, lde, item2ent, n_items, pref_ws, g.ppad, g.dp, n_pref, d, tables, &t, st, name)) return rc;
  a.A = t.A; a.SCU = t.SCU; a.B = t.B;
  if (filt_off) {
    if (int rc = sweep_filter_bits(filt_off, filt_ids, nq, n_items, bm, a.bm_words, st, name)) return rc;
    a.bm = bm;
  }
  if (d == 64) return launch_pref_rank_p<16>(n_pref, a, st, name);
  if (d == 100) return launch_pref_rank_p<25>(n_pref, a, st, name);
  return launch_pref_rank_p<32>(n_pref, a, st, name);
}
