// The one-sweep filtered top-n pass that dot_pass_kernel (ktup_dot_pass.hip) and cfkg_pass_kernel (ktup_cfkg.hip) share: scores of
// every (user, candidate) pair AND the filtered top-n of every user in ONE sweep that never writes the (users x candidates) matrix.
//   * a workgroup owns 64 users (4 waves x 16) and a contiguous split of the candidates.  A wave keeps its 16 users' query rows in
//     REGISTERS for the whole pass (one float per lane and 4 k); candidate rows stream through a double-buffered LDS stage (rows at
//     an odd float4 pitch: the B operand reads of a 16-candidate tile hit 64 different banks; what else a candidate carries rides in
//     the row's last, spare slot) that the next stage's global loads refill under the arithmetic.  Every 16-candidate tile of a stage
//     has an accumulator of its own;
//   * ranking: a user's sorted top-n list (64-bit keys = order-preserving image of the NEGATED score << 32 | candidate: descending
//     score, ties -> lower candidate, the order of ktup_rank.hip with descending = 1) lives in the wave's LDS and is touched only
//     when 16 candidates are pending for it.  A score is a candidate if it beats the user's n-th score (one float compare; the keys
//     decide equality, NaNs and a list that is still short) and its bit in the pass's filter bitmap (built once per pass from the CSR
//     lists, read from L2 by candidates only) is clear;
//   * the splits' partial lists are merged by a last, tiny launch (topk_merge_kernel, ktup_topn.h).
// The list has two widths (ktup_topn.h): SEG = 1, one key per lane of the user's 16-lane row (topn <= 16), is what the narrow entry
// points launch; SEG = 2 and 4 (topn <= 32, <= 64) are the wide entry points' (ktup_eval_dot_topk_wide, ktup_eval_cfkg_topk_wide).
// A wide list costs 2 or 6 KB more LDS per wave and a longer merge network; scorers, stages, filter bits, pending rows and the
// append are the same code, so a score is the same bits at every width.  The sweeps of TUP / KTUP (ktup_eval_pass.hip,
// ktup_eval.hip) have pass bodies of their own; the first keeps its lists in the same segments.  Measured against the batch walk, which was all there was above 16
// (profiles/wide_topn_times.txt, whole pass through the driver): inner products 6040 x 3240, d = 64: topn 20 0.85 -> 0.25 ms, topn 50
// 1.52 -> 0.49 ms; 512 x 100,000: 1.65 -> 0.46 and 3.40 -> 1.05 ms; CFKG at d = 100: 1.31 -> 0.84 (L1) and 1.19 -> 0.65 ms (squared
// L2) at topn 20.  The registers of a wide kernel are bounded for the workgroups per CU its LDS admits (sweep_wide_wgs); no wide
// instantiation spills.
// Here live, ONCE: the geometry, the pass body (sweep_pass), the split rule, the workspace layout, the filter bitmap, the launch
// ladder over the row width and the merge launch.  What a model adds is its SCORER, a small type that supplies
//     static constexpr size_t LDS                       bytes of its own between the stages and the waves' lists (a multiple of 16)
//     float query(u, k)                                 element k of user row u's query row
//     void hold(av, smem, u0, in, kq, j)                what it keeps of the wave's query rows av[KS] for the pass
//     const float* row(c, live)                         candidate c's table row (one that may be read if it has none: live = false)
//     v4 spare(c, live)                                 what rides in the candidate's spare slot
//     void tile_math(av, eb, kq, acc)                   the stage's arithmetic: acc[t][reg] of user 4 kq + reg x candidate 16 t + j
//     staged(slot)                                      what it reads back of a staged candidate's spare slot, and from that
//     bool live(spare), float score(acc, reg, spare)    whether the candidate is ranked at all; its score (descending)
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <type_traits>

#include "ktup_common.h"
#include "ktup_lane_swap.h"
#include "ktup_topn.h"

namespace ktup {

// The filter lists of a pass as bits (ktup_sweep_pass.hip): bm[b * words + (id >> 5)] bit (id & 31) for every id in [0, n) of user
// b's list, all other bits 0
int sweep_filter_bits(const int64_t* off, const int32_t* ids, int64_t nq, int64_t n, uint32_t* bm, int64_t words, hipStream_t st,
                      const char* name);

namespace {

constexpr int NSPLIT_MAX = 32;   // candidate splits: NSPLIT_MAX * TOPN_MAX keys per user is what the merge holds, eight per lane
constexpr int MERGE_PER_LANE = NSPLIT_MAX * TOPN_MAX / 64;
// the split rule: 512 / topn splits, at most 32 -- 32 up to topn 16, 25 at 20, 10 at 50, 8 at 64
constexpr int sweep_max_splits(int topn) { return 64 * MERGE_PER_LANE / topn < NSPLIT_MAX ? 64 * MERGE_PER_LANE / topn : NSPLIT_MAX; }
constexpr size_t wave_lds(int seg) { return (size_t)16 * PCAP * 8 + (size_t)16 * 16 * seg * 8; }   // pending rows | lists of seg 16-key segments
constexpr int sweep_segments(int topn) { return topn <= 32 ? 2 : 4; }   // the wide entry points' list width
constexpr size_t SWEEP_LDS_MAX = 160 * 1024;
// the workgroups per CU a wide kernel's registers are bounded for: two where two fit the LDS, else one (and 512 registers a lane)
constexpr int sweep_wide_wgs(size_t lds) { return 2 * lds <= SWEEP_LDS_MAX ? 2 : 1; }

struct SweepArgs {
  const int64_t* u_ids; int64_t nq, n;  // the users' rows; users and candidates of the pass
  int d, vec;                           // vec: candidate rows are whole, 16-byte aligned float4 (else element by element)
  const uint32_t* bm; int64_t bm_words; // the filter bits [nq][bm_words]; NULL = no filter
  int topn, nsplit; int64_t split;      // candidates per split
  uint64_t* part;                       // [nq][nsplit][topn] partial lists
};

// KS: 4-wide k steps (d <= 4 KS; the padding holds zeros on both sides: fma(0, 0, acc) = acc, a chain that starts at +0 never holds
// -0, and it adds nothing to a distance)
// STC: candidates per stage where a kernel cannot afford the usual ones (0: 64, or 32 for the wide rows)
template <int KS, int STC = 0>
struct SweepGeom {
  static constexpr int ST = STC ? STC : KS > 32 ? 32 : 64;   // candidates per stage
  static constexpr int NSUB = ST / 16;               // 16-candidate tiles per stage = accumulators per wave
  static constexpr int CPR = KS + 1;                 // float4 slots per row: KS operand quads + the spare slot
  static constexpr int ROW4 = CPR | 1;               // the row's float4 pitch in LDS: odd
  static constexpr int STG = ST * ROW4;              // float4 per stage buffer
  static constexpr int SLOTS = ST * KS;              // operand quads a stage loads
  static constexpr int NPRE = (SLOTS + 255) / 256;   // float4 per thread in flight for the next stage
  static constexpr size_t STAGES = (size_t)2 * STG * 16;
  static constexpr size_t lds(size_t scorer, int seg = 1) { return STAGES + scorer + 4 * wave_lds(seg); }   // stages | the scorer's | pending rows and lists
};

// ---- device side -----------------------------------------------------------------------------
// The pass of one workgroup (256 threads, SweepGeom<KS, STC>::lds(S::LDS, SEG) bytes at smem); SEG: 16-key segments of a user's list.
template <int KS, bool VEC, int SEG = 1, int STC = 0, class S>
KTUP_DEV void sweep_pass(const SweepArgs& a, S& sc, char* smem) {
  using G = SweepGeom<KS, STC>;
  constexpr int ST = G::ST, NSUB = G::NSUB, ROW4 = G::ROW4, STG = G::STG, SLOTS = G::SLOTS, NPRE = G::NPRE;
  v4* Xb = reinterpret_cast<v4*>(smem);                                   // [2][STG] candidate stages
  const int tid = threadIdx.x, lane = tid & 63, kq = lane >> 4, j = lane & 15;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  uint64_t* pbuf = reinterpret_cast<uint64_t*>(smem + G::STAGES + S::LDS + (size_t)w * wave_lds(SEG));   // [16][PCAP] pending candidates
  uint64_t* tk = pbuf + 16 * PCAP;                                        // [16][SEG][16] the users' sorted lists (touched by merges only)
  const int64_t ub = (int64_t)(blockIdx.x / (unsigned)a.nsplit);
  const int sp = (int)(blockIdx.x - (unsigned)ub * (unsigned)a.nsplit);
  const int64_t u0 = ub * 64 + 16 * w;
  const int64_t i_lo = (int64_t)sp * a.split;
  const int64_t i_hi = min(a.n, i_lo + a.split);
  const int topn = a.topn, d = a.d;
  for (int idx = lane; idx < 16 * 16 * SEG; idx += 64) tk[idx] = PKEY_MAX;
  // A operands of the whole pass: lane (kq, j) holds element 4 s + kq of user j's query row for every k step s
  float av[KS];
  {
    const bool ok = u0 + j < a.nq;
    const int64_t u = ok ? a.u_ids[u0 + j] : 0;
#pragma unroll
    for (int s = 0; s < KS; ++s) av[s] = sc.query(u, min(4 * s + kq, d - 1));   // (unconditional, from clamped addresses: all in flight together)
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int s = 0; s < KS; ++s) av[s] = (ok && 4 * s + kq < d) ? av[s] : 0.f;
  }
  uint64_t thr[4];                                                        // the users' n-th keys (rows past the end: nothing is ever below)
  // ... and their scores: a score above is a candidate, one below is not -- one float compare per score; an equal score, a NaN on
  // either side (the threshold of a list that is still short is one) or a zero of the other sign goes through the 64-bit key
  // compare, so the order is that of the keys in every case
  float thrf[4];
  int pend[4] = {0, 0, 0, 0};
  bool in[4];   // the user of this lane's accumulator row reg is one of the pass (made once: each further copy of these compares is an SGPR pair)
#pragma unroll
  for (int reg = 0; reg < 4; ++reg) {
    in[reg] = u0 + 4 * kq + reg < a.nq;
    thr[reg] = in[reg] ? PKEY_MAX : 0ull;
    thrf[reg] = in[reg] ? __uint_as_float(0x7fffffffu) : __builtin_inff();
  }
  sc.hold(av, smem + G::STAGES, u0, in, kq, j);                          // (what it writes to LDS is read after the workgroup barrier below)
  // ---- the stage loads: slot e of a stage = operand quad c of candidate r (r = e / KS); candidates past the end re-read the last
  // one, candidates without a row read one that is there (both are masked out below, the operands only have to be there).
  // Straight-line code: every load is unconditional from a clamped address and zeroed by a select where it is padding, so that all
  // loads of a stage are in flight together (with a branch per slot the compiler waited for each load before the next: 17 round
  // trips per stage).  The spare slot is loaded by the first ST threads.
  v4 pre[NPRE];
  v4 pre_spare = {0.f, 0.f, 0.f, 0.f};
  auto fetch = [&](int64_t row0) __attribute__((always_inline)) {
#pragma unroll
    for (int k = 0; k < NPRE; ++k) {
      const int e = min(tid + 256 * k, SLOTS - 1);
      const int r = e / KS, c = e - r * KS;
      bool live;
      const float* row = sc.row(min(row0 + r, a.n - 1), live);
      if constexpr (VEC) {
        pre[k] = *reinterpret_cast<const v4*>(row + min(4 * c, d - 4));
      } else {
#pragma unroll
        for (int q = 0; q < 4; ++q) pre[k][q] = row[min(4 * c + q, d - 1)];
      }
    }
    const int64_t mine = min(row0 + min(tid, ST - 1), a.n - 1);
    bool live;
    (void)sc.row(mine, live);
    pre_spare = sc.spare(mine, live);
  };
  auto stash = [&](int buf) __attribute__((always_inline)) {
#pragma unroll
    for (int k = 0; k < NPRE; ++k) {
      const int e = tid + 256 * k;
      if (e >= SLOTS) continue;
      const int r = e / KS, c = e - r * KS;
      v4 v = pre[k];                                                       // (the padding is zeroed here, not at the load: a select on
      if (d != 4 * KS) {                                                   //  the loaded value would wait for it before the arithmetic)
#pragma unroll
        for (int q = 0; q < 4; ++q) v[q] = 4 * c + q < d ? v[q] : 0.f;
      }
      Xb[buf * STG + r * ROW4 + c] = v;
    }
    if (tid < ST) Xb[buf * STG + tid * ROW4 + KS] = pre_spare;
  };
  // ---- ranking: candidates are appended to the user's pending row in LDS at positions taken from a ballot (`pend` is replicated
  // over the row's 16 lanes); once a row of a register slot holds 16, that slot's four rows go through the merge network and the
  // n-th keys are renewed
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
      uint64_t merged;                                                                // the segment that holds the n-th key
      if constexpr (SEG == 1) {
        merged = row_merge_pending(tk[ur * 16 + j], row, n, topn, j);                 // all four rows of the slot at once
        tk[ur * 16 + j] = merged;
      } else {
        uint64_t* lst = tk + ur * 16 * SEG + j;
        uint64_t seg[SEG];
#pragma unroll
        for (int s = 0; s < SEG; ++s) seg[s] = lst[16 * s];
        row_merge_pending_wide<SEG>(seg, row, n, topn, j);
        merged = seg[0];
#pragma unroll
        for (int s = 0; s < SEG; ++s) {
          lst[16 * s] = seg[s];
          if (s == (topn - 1) >> 4) merged = seg[s];
        }
      }
      pend[reg] = 0;
      const int nth = SEG == 1 ? rowbase + topn - 1 : rowbase + ((topn - 1) & 15);
      const uint32_t nhi = (uint32_t)__shfl((int)(uint32_t)(merged >> 32), nth, 64);
      const uint32_t nlo = (uint32_t)__shfl((int)(uint32_t)merged, nth, 64);
      if (in[reg]) {                                                                  // (rows past the end keep 0 / +inf)
        thr[reg] = ((uint64_t)nhi << 32) | nlo;
        thrf[reg] = -topn_key_score(nhi);                                               // negated back (NaN: list short)
      }
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
  };
  auto rank_tile = [&](const v4& acc, const v4* slot, int64_t cand) __attribute__((always_inline)) {   // 16 users x the 16 candidates [cand - j, cand - j + 16)
    const auto spare = sc.staged(slot);
    const bool iok = cand < i_hi && sc.live(spare);
    bool full = false;
#pragma unroll
    for (int reg = 0; reg < 4; ++reg) {
      const int ur = 4 * kq + reg;
      const float s = sc.score(acc[reg], reg, spare);
      const bool above = s > thrf[reg], maybe = !(s < thrf[reg]) && iok;
      if (!__builtin_amdgcn_ballot_w64(maybe)) continue;                   // most 64-score slots leave here
      const uint64_t key = topn_key(s, true, (uint32_t)cand);
      bool c = maybe && (above || key < thr[reg]);
      if (c && a.bm) c = ((a.bm[(u0 + ur) * a.bm_words + (cand >> 5)] >> (cand & 31)) & 1u) == 0u;
      const uint64_t m = __builtin_amdgcn_ballot_w64(c);
      if (m) {
        app.put(pbuf, ur * PCAP, pend[reg], m, c, [&] { return key; });
        full |= pend[reg] >= 16;
      }
    }
    if (__builtin_amdgcn_ballot_w64(full)) flush(false);
  };
  auto compute = [&](int buf, int64_t row0) __attribute__((always_inline)) {
    const v4* eb = Xb + buf * STG + j * ROW4;                              // candidate j of tile 0
    v4 acc[NSUB];
#pragma unroll
    for (int t = 0; t < NSUB; ++t) acc[t] = (v4){0.f, 0.f, 0.f, 0.f};
    sc.tile_math(av, eb, kq, acc);
#pragma unroll
    for (int t = 0; t < NSUB; ++t) {
      if (row0 + 16 * t >= i_hi) break;                                    // (uniform)
      rank_tile(acc[t], eb + t * 16 * ROW4 + KS, row0 + 16 * t + j);
    }
  };
  const int64_t nst = (i_hi - i_lo + ST - 1) / ST;
  fetch(i_lo);
  stash(0);
  __syncthreads();                                                         // stage 0, what the scorer holds in LDS and the lists are in place
  // one stage per workgroup barrier; the next stage's loads are in flight under this stage's arithmetic.  Buffer buf ^ 1 was last read
  // in the previous iteration, whose closing barrier every wave has passed; its new contents are read after this iteration's barrier.
  for (int64_t t0 = 0; t0 < nst; ++t0) {
    const int buf = (int)(t0 & 1);
    const bool more = t0 + 1 < nst;
    if (more) fetch(i_lo + (t0 + 1) * ST);
    __builtin_amdgcn_sched_barrier(0);                                     // the loads are issued before, their values used after the arithmetic
    compute(buf, i_lo + t0 * ST);
    __builtin_amdgcn_sched_barrier(0);
    if (more) stash(buf ^ 1);
    __syncthreads();
  }
  flush(true);
  if constexpr (SEG == 1) {                                                // (the loop below with SEG = 1, as it was written for the narrow
    if (j < topn) {                                                        //  lists alone: through the loop the same stores come out of
#pragma unroll                                                             //  another register allocation)
      for (int reg = 0; reg < 4; ++reg) {
        const int64_t ur = u0 + 4 * kq + reg;
        if (ur < a.nq) a.part[(ur * a.nsplit + sp) * topn + j] = tk[(4 * kq + reg) * 16 + j];
      }
    }
  } else {
#pragma unroll
    for (int s = 0; s < SEG; ++s) {
      const int p = 16 * s + j;                                            // this lane's key of segment s
      if (p >= topn) continue;
#pragma unroll
      for (int reg = 0; reg < 4; ++reg) {
        const int64_t ur = u0 + 4 * kq + reg;
        if (ur < a.nq) a.part[(ur * a.nsplit + sp) * topn + p] = tk[(4 * kq + reg) * 16 * SEG + p];
      }
    }
  }
}

// The dot products of a stage on v_mfma_f32_16x16x4_f32, k ascending: fp32 in, fp32 accumulate, per accumulator the fmaf chain of
// the K11 kernel (bprmf_eval_kernel).  Independent MFMA chains per wave.
template <int KS>
KTUP_DEV void sweep_tile_dot(const float (&av)[KS], const v4* eb, int kq, v4 (&acc)[SweepGeom<KS>::NSUB]) {
  constexpr int ROW4 = SweepGeom<KS>::ROW4;
  const float* rb = reinterpret_cast<const float*>(eb) + kq;               // lane (kq, candidate j): element kq of every k quad
#pragma unroll
  for (int s = 0; s < KS; ++s) {
#pragma unroll
    for (int t = 0; t < SweepGeom<KS>::NSUB; ++t)
      acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[s], rb[t * 16 * ROW4 * 4 + 4 * s], acc[t], 0, 0, 0);
  }
}

// ---- host side -------------------------------------------------------------------------------
// how the candidates are cut: `want` splits, whole 16-candidate tiles each.  0: about 1.25 workgroups per CU.  Every split keeps a
// list of its own per user, so more splits mean more candidates through the append / merge path and a prologue each; fewer leave CUs
// idle.  Measured (one MI355X, inner products, d = 64, topn 10, ~165 filtered ids per user, whole call): 6040 x 3240: 4 splits 143 us
// (1: 260, 8: 165, 12: 189); 512 x 100,000: 32 splits 279 us (16: 431, 8: 710); 30,000 x 25,000: 1 split 1.76 ms (3: 2.09, 8: 2.50).
// At most sweep_max_splits(topn): what the merge kernel holds.
inline int sweep_nsplit(int64_t nq, int64_t n, int topn, int want, int64_t* split) {
  const int64_t nub = (nq + 63) / 64;
  const int64_t cap = sweep_max_splits(topn);
  int64_t ns = want > 0 ? want : (320 + nub - 1) / (nub > 0 ? nub : 1);
  ns = ns < 1 ? 1 : ns > cap ? cap : ns;
  int64_t si = (n + ns - 1) / ns;
  si = (si + 15) / 16 * 16;
  if (want <= 0 && si < 256) si = 256;                                     // (a workgroup's prologue wants some candidates to pay for it)
  *split = si;
  return (int)((n + si - 1) / si);
}

// workspace: the partial lists (8-byte entries, so the bits start on an 8-byte boundary) | the filter bits | cand_floats floats per
// candidate.  0 for sizes no pass runs with (topn_max: TOPN_MAX, or TOPN_WIDE_MAX for the wide entry points).
inline size_t sweep_workspace_bytes(int64_t nq, int64_t n, int topn, int topn_max, int nsplit, int cand_floats) {
  if (nq <= 0 || n <= 0 || topn <= 0 || topn > topn_max || nsplit < 0) return 0;
  int64_t si = 0;
  const int ns = sweep_nsplit(nq, n, topn, nsplit, &si);
  const size_t part = (size_t)nq * ns * topn * sizeof(uint64_t);
  const size_t bits = (size_t)nq * (size_t)((n + 31) / 32) * sizeof(uint32_t);
  return part + bits + (size_t)cand_floats * n * sizeof(float) + 16;
}

// Cuts the candidates and the workspace and builds the filter bits of a pass whose a.u_ids, nq, n, d, vec and topn are set;
// *cand_floats (optional): the per-candidate floats of the workspace.
inline int sweep_prepare(SweepArgs& a, int nsplit, const int64_t* filt_off, const int32_t* filt_ids, void* ws, float** cand_floats,
                         hipStream_t st, const char* name) {
  a.nsplit = sweep_nsplit(a.nq, a.n, a.topn, nsplit, &a.split);
  a.part = reinterpret_cast<uint64_t*>(ws);
  a.bm = nullptr;
  a.bm_words = (a.n + 31) / 32;
  if ((a.nq + 63) / 64 * a.nsplit > 0x7fffffffLL)
    return set_error(KTUP_ERR_UNSUPPORTED, "%s: too many users for one call (%lld)", name, (long long)a.nq);
  uint32_t* bm = reinterpret_cast<uint32_t*>(a.part + (size_t)a.nq * a.nsplit * a.topn);
  if (cand_floats) *cand_floats = reinterpret_cast<float*>(bm + a.nq * a.bm_words);
  if (filt_off) {
    if (int rc = sweep_filter_bits(filt_off, filt_ids, a.nq, a.n, bm, a.bm_words, st, name)) return rc;
    a.bm = bm;
  }
  return KTUP_OK;
}

// f(std::integral_constant<int, KS>) with the narrowest compiled row width that holds d floats
template <typename F>
inline int with_k_steps(int d, F f) {
  const int nk = (d + 3) / 4;
  if (nk <= 5) return f(std::integral_constant<int, 5>{});
  if (nk <= 9) return f(std::integral_constant<int, 9>{});
  if (nk <= 16) return f(std::integral_constant<int, 16>{});
  if (nk <= 25) return f(std::integral_constant<int, 25>{});
  if (nk <= 32) return f(std::integral_constant<int, 32>{});
  if (nk <= 48) return f(std::integral_constant<int, 48>{});
  return f(std::integral_constant<int, 64>{});
}

// one workgroup per (64 users, split)
template <size_t LDS, class Args>
int sweep_launch(void (*kernel)(Args), const Args& args, const SweepArgs& a, hipStream_t st, const char* name) {
  static_assert(LDS <= SWEEP_LDS_MAX, "the stages, what the scorer holds and the lists fit the LDS");
  (void)hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)LDS);
  hipLaunchKernelGGL(kernel, dim3((unsigned)((a.nq + 63) / 64 * a.nsplit)), dim3(256), LDS, st, args);
  return check_launch(name);
}

// the splits' partial lists -> top_ids / top_scores (NEGATE: ktup_topn.h)
template <bool NEGATE>
int sweep_merge(const SweepArgs& a, int32_t* top_ids, float* top_scores, hipStream_t st, const char* name) {
  hipLaunchKernelGGL((topk_merge_kernel<MERGE_PER_LANE, NEGATE>), dim3((unsigned)((a.nq + 3) / 4)), dim3(MERGE_T), 0, st, a.part, a.nq, a.nsplit,
                     a.topn, top_ids, top_scores);
  return check_launch(name);
}

}  // namespace
}  // namespace ktup
