// The filtered rank of EVERY gold item of a rec evaluation pass in one sweep that never writes the (users x candidates) matrix:
// ktup_eval_dot_ranks (BPRMF, FM, CKE, coFM) and ktup_eval_cfkg_ranks -- what ktup_eval_gold_ranks returns on the scores of
// ktup_eval_dot_topk / ktup_eval_cfkg_topk, the counterpart of ktup_eval_kg_ranks_fused on the rec side (mean rank, MRR and AUC need
// the place of every held-out item, not the first n of the list).
//
// A rank is a COUNT: rank(g) = #{candidates of the user ordered before g that are neither filtered nor gold}, the order being the list
// passes' 64-bit key (ktup_topn.h topn_key: descending score, ties -> lower candidate).  Two launches on the scorers of the list
// passes (ktup_sweep_scorers.h: the same tile_math / score / live, so the same score bits):
//   * rank_keys_kernel, one workgroup per 64 users: the block's concatenated gold lists gold_ids[gold_off[64 b] .. gold_off[64 b + 64])
//     stream through the stages AS the candidate list -- the sweep's own instruction sequence on rows gathered by id -- and lane
//     (user, entry) keeps the key where the entry lies in that user's own range.  A gold that is filtered, outside [0, n) or without
//     a row gets "no key" (above every real one) and the rank -1; all others get 0.  The keys are sorted per user (by counting) and
//     written with their permutation to the workspace;
//   * rank_count_kernel, one workgroup per (64 users, candidate split): query rows in registers, the double-buffered LDS stage,
//     straight-line stage loads and filter bits read by survivors only, as sweep_pass; instead of pending rows and sorted lists the
//     LDS holds the block's sorted gold keys and one 32-bit counter per gold slot.  A score that does not beat the user's worst gold
//     leaves after one float compare and one ballot; a survivor builds its key, reads its filter bit, finds by binary search how
//     many of the user's gold keys are ordered before it (an equal key is the gold itself: skipped) and bumps that bucket with an
//     LDS integer add.  The prefix sums over a user's buckets are the split's partial ranks, added to `ranks` with integer global
//     atomics: exact in any order, so a rank is the same integer at every nsplit.  No float atomics.
// The stage loop (rank_stream) is a body of its own beside sweep_pass: the list kernels keep their machine code
// (profiles/rec_ranks_narrow_check.txt).
#include "ktup_cfkg_norm.h"
#include "ktup_sweep_scorers.h"

namespace ktup {
namespace {

// gold entries of a 64-user block the LDS holds beside the two stages and what the scorer keeps (include/ktup_hip.h states the cap)
constexpr int rank_cap(int ks) { return ks <= 32 ? KTUP_RANK_BLOCK_GOLDS : KTUP_RANK_BLOCK_GOLDS_WIDE; }
constexpr int rank_cap_d(int d) { return rank_cap((d + 3) / 4); }
constexpr size_t RANK_OFF_BYTES = 80 * sizeof(int);                       // the block's 65 offsets
// offsets | gcap sorted keys | gcap counters
constexpr size_t rank_gold_lds(int64_t gcap) { return RANK_OFF_BYTES + (size_t)gcap * (sizeof(uint64_t) + sizeof(uint32_t)); }

struct RankArgs {
  const int64_t* u_ids; int64_t nq, n;  // the users' rows; users and candidates of the pass
  int d;
  const uint32_t* bm; int64_t bm_words; // the filter bits [nq][bm_words]; NULL = no filter
  const int64_t* gold_off; const int32_t* gold_ids;
  uint64_t* skey;                       // [n_gold] every user's gold keys, ascending ("no key" last)
  int32_t* perm;                        // [n_gold] which entry of the block (relative to its first) the sorted slot holds
  int32_t* ranks;
  int gcap;                             // gold entries per block the launch's LDS holds (a multiple of 64)
  int nsplit; int64_t split;            // candidates per split
};

template <class MA>
struct RankKernelArgs { MA m; RankArgs r; };

// the workgroups per CU the registers are bounded for: two where two workgroups with the smallest gold area fit the LDS, else one
template <class S, int KS>
constexpr int rank_wgs() { return sweep_wide_wgs(SweepGeom<KS>::STAGES + S::LDS + rank_gold_lds(64)); }

// candidate e of the key launch: the row, the liveness and the spare slot of candidate gold_ids[e]
template <class S>
struct GoldRows {
  const S& sc; const int32_t* ids; int64_t n;
  KTUP_DEV const float* row(int64_t e, bool& live) const {
    const int64_t id = ids[e];
    const bool ok = id >= 0 && id < n;
    const float* p = sc.row(ok ? id : (int64_t)0, live);
    live = live && ok;
    return p;
  }
  KTUP_DEV v4 spare(int64_t e, bool live) const {
    const int64_t id = ids[e];
    return sc.spare(id >= 0 && id < n ? id : (int64_t)0, live);
  }
};

// The stream of one workgroup (256 threads): candidates [i_lo, i_hi) of `rows` (clamped to n - 1) past the 16 users of every wave,
// tile(acc, slot, cand) for lane (kq, j) of every 16-candidate tile: acc[reg] = what tile_math made of user 4 kq + reg x candidate
// cand, slot = the candidate's staged spare slot.  Geometry, query rows, stage loads and the barrier scheme are sweep_pass's.
template <int KS, bool VEC, class Rows, class S, class Tile>
KTUP_DEV void rank_stream(const RankArgs& a, const Rows& rows, S& sc, char* smem, int64_t u0, const bool (&in)[4], int64_t i_lo, int64_t i_hi,
                          int64_t n, Tile tile) {
  using G = SweepGeom<KS>;
  constexpr int ST = G::ST, NSUB = G::NSUB, ROW4 = G::ROW4, STG = G::STG, SLOTS = G::SLOTS, NPRE = G::NPRE;
  v4* Xb = reinterpret_cast<v4*>(smem);                                   // [2][STG] candidate stages
  const int tid = threadIdx.x, lane = tid & 63, kq = lane >> 4, j = lane & 15;
  const int d = a.d;
  float av[KS];
  {
    const bool ok = u0 + j < a.nq;
    const int64_t u = ok ? a.u_ids[u0 + j] : 0;
#pragma unroll
    for (int s = 0; s < KS; ++s) av[s] = sc.query(u, min(4 * s + kq, d - 1));
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int s = 0; s < KS; ++s) av[s] = (ok && 4 * s + kq < d) ? av[s] : 0.f;
  }
  sc.hold(av, smem + G::STAGES, u0, in, kq, j);
  v4 pre[NPRE];
  v4 pre_spare = {0.f, 0.f, 0.f, 0.f};
  auto fetch = [&](int64_t row0) __attribute__((always_inline)) {
#pragma unroll
    for (int k = 0; k < NPRE; ++k) {
      const int e = min(tid + 256 * k, SLOTS - 1);
      const int r = e / KS, c = e - r * KS;
      bool live;
      const float* row = rows.row(min(row0 + r, n - 1), live);
      if constexpr (VEC) {
        pre[k] = *reinterpret_cast<const v4*>(row + min(4 * c, d - 4));
      } else {
#pragma unroll
        for (int q = 0; q < 4; ++q) pre[k][q] = row[min(4 * c + q, d - 1)];
      }
    }
    const int64_t mine = min(row0 + min(tid, ST - 1), n - 1);
    bool live;
    (void)rows.row(mine, live);
    pre_spare = rows.spare(mine, live);
  };
  auto stash = [&](int buf) __attribute__((always_inline)) {
#pragma unroll
    for (int k = 0; k < NPRE; ++k) {
      const int e = tid + 256 * k;
      if (e >= SLOTS) continue;
      const int r = e / KS, c = e - r * KS;
      v4 v = pre[k];
      if (d != 4 * KS) {
#pragma unroll
        for (int q = 0; q < 4; ++q) v[q] = 4 * c + q < d ? v[q] : 0.f;
      }
      Xb[buf * STG + r * ROW4 + c] = v;
    }
    if (tid < ST) Xb[buf * STG + tid * ROW4 + KS] = pre_spare;
  };
  auto compute = [&](int buf, int64_t row0) __attribute__((always_inline)) {
    const v4* eb = Xb + buf * STG + j * ROW4;
    v4 acc[NSUB];
#pragma unroll
    for (int t = 0; t < NSUB; ++t) acc[t] = (v4){0.f, 0.f, 0.f, 0.f};
    sc.tile_math(av, eb, kq, acc);
#pragma unroll
    for (int t = 0; t < NSUB; ++t) {
      if (row0 + 16 * t >= i_hi) break;                                    // (uniform)
      tile(acc[t], eb + t * 16 * ROW4 + KS, row0 + 16 * t + j);
    }
  };
  const int64_t nst = (i_hi - i_lo + ST - 1) / ST;
  fetch(i_lo);
  stash(0);
  __syncthreads();                                                         // stage 0, what the scorer and the caller put in LDS are in place
  for (int64_t t0 = 0; t0 < nst; ++t0) {
    const int buf = (int)(t0 & 1);
    const bool more = t0 + 1 < nst;
    if (more) fetch(i_lo + (t0 + 1) * ST);
    __builtin_amdgcn_sched_barrier(0);
    compute(buf, i_lo + t0 * ST);
    __builtin_amdgcn_sched_barrier(0);
    if (more) stash(buf ^ 1);
    __syncthreads();
  }
}

// the block's gold range and, in LDS, its users' offsets relative to it (users past the end: empty ranges at the end)
struct RankBlock { int64_t g_lo; int64_t G; };
KTUP_DEV RankBlock rank_block(const RankArgs& a, int64_t ub, int* goff) {
  const int64_t b0 = ub * 64;
  const int64_t g_lo = a.gold_off[b0];
  const int64_t G = a.gold_off[min(a.nq, b0 + 64)] - g_lo;
  if (G > 0 && G <= a.gcap && threadIdx.x <= 64) goff[threadIdx.x] = (int)(a.gold_off[min(a.nq, b0 + (int64_t)threadIdx.x)] - g_lo);
  return RankBlock{g_lo, G};
}

template <class S, int KS, bool VEC, class MA>
__global__ __launch_bounds__(256, (rank_wgs<S, KS>())) void rank_keys_kernel(RankKernelArgs<MA> ka) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  using G = SweepGeom<KS>;
  const RankArgs& a = ka.r;
  int* goff = reinterpret_cast<int*>(smem + G::STAGES + S::LDS);
  uint64_t* gk = reinterpret_cast<uint64_t*>(smem + G::STAGES + S::LDS + RANK_OFF_BYTES);
  const int tid = threadIdx.x, lane = tid & 63, kq = lane >> 4;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int64_t ub = blockIdx.x;
  const RankBlock blk = rank_block(a, ub, goff);
  if (blk.G <= 0) return;                                                  // (uniform exits: before every barrier)
  if (blk.G > a.gcap) {                                                    // more than the caller announced: nothing of the block is ranked
    for (int64_t e = tid; e < blk.G; e += 256) a.ranks[blk.g_lo + e] = -1;
    return;
  }
  const int64_t g_lo = blk.g_lo, g_hi = g_lo + blk.G;
  __syncthreads();
  const int64_t u0 = ub * 64 + 16 * w;
  bool in[4];
  int lo[4], hi[4];
#pragma unroll
  for (int reg = 0; reg < 4; ++reg) {
    in[reg] = u0 + 4 * kq + reg < a.nq;
    lo[reg] = goff[16 * w + 4 * kq + reg];
    hi[reg] = goff[16 * w + 4 * kq + reg + 1];
  }
  S sc{ka.m};
  const GoldRows<S> rows{sc, a.gold_ids, a.n};
  rank_stream<KS, VEC>(a, rows, sc, smem, u0, in, g_lo, g_hi, g_hi, [&](const v4& acc, const v4* slot, int64_t e) __attribute__((always_inline)) {
    const auto spare = sc.staged(slot);
    const bool eok = e < g_hi;
    const int64_t id = a.gold_ids[min(e, g_hi - 1)];
    const bool ranked = id >= 0 && id < a.n && sc.live(spare);
    const int rel = (int)(e - g_lo);
#pragma unroll
    for (int reg = 0; reg < 4; ++reg) {
      if (!(eok && rel >= lo[reg] && rel < hi[reg])) continue;            // the entry is this user's own
      const float s = sc.score(acc[reg], reg, spare);
      bool v = ranked;
      if (v && a.bm) v = ((a.bm[(u0 + 4 * kq + reg) * a.bm_words + (id >> 5)] >> (id & 31)) & 1u) == 0u;
      gk[rel] = v ? topn_key(s, true, (uint32_t)id) : PKEY_MAX;
    }
  });
  // (the stream's last barrier is behind every wave: all keys are in place)  A wave sorts its 16 users' keys by counting: equal keys
  // -- an id that occurs twice -- stay in entry order
  for (int ur = 16 * w; ur < 16 * w + 16; ++ur) {
    const int l0 = goff[ur], l1 = goff[ur + 1];
    for (int i = l0 + lane; i < l1; i += 64) {
      const uint64_t k = gk[i];
      int pos = 0;
      for (int o = l0; o < l1; ++o) {
        const uint64_t ko = gk[o];
        pos += (ko < k || (ko == k && o < i)) ? 1 : 0;
      }
      a.skey[g_lo + l0 + pos] = k;
      a.perm[g_lo + l0 + pos] = i;
      a.ranks[g_lo + i] = k == PKEY_MAX ? -1 : 0;
    }
  }
}

template <class S, int KS, bool VEC, class MA>
__global__ __launch_bounds__(256, (rank_wgs<S, KS>())) void rank_count_kernel(RankKernelArgs<MA> ka) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  using G = SweepGeom<KS>;
  const RankArgs& a = ka.r;
  int* goff = reinterpret_cast<int*>(smem + G::STAGES + S::LDS);
  uint64_t* gk = reinterpret_cast<uint64_t*>(smem + G::STAGES + S::LDS + RANK_OFF_BYTES);
  uint32_t* cnt = reinterpret_cast<uint32_t*>(gk + a.gcap);
  const int tid = threadIdx.x, lane = tid & 63, kq = lane >> 4;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int64_t ub = (int64_t)(blockIdx.x / (unsigned)a.nsplit);
  const int sp = (int)(blockIdx.x - (unsigned)ub * (unsigned)a.nsplit);
  const RankBlock blk = rank_block(a, ub, goff);
  if (blk.G <= 0 || blk.G > a.gcap) return;                                // (uniform: before every barrier)
  const int64_t g_lo = blk.g_lo;
  for (int i = tid; i < (int)blk.G; i += 256) {
    gk[i] = a.skey[g_lo + i];
    cnt[i] = 0u;
  }
  __syncthreads();
  const int64_t u0 = ub * 64 + 16 * w;
  const int64_t i_lo = (int64_t)sp * a.split;
  const int64_t i_hi = min(a.n, i_lo + a.split);
  // per accumulator row: where the user's keys start, how many are real, the worst of them and its score (no real key: nothing is
  // ever ordered before -- key 0 / +inf, as the list pass's rows past the end)
  bool in[4];
  int lo[4], nv[4];
  uint64_t thr[4];
  float thrf[4];
#pragma unroll
  for (int reg = 0; reg < 4; ++reg) {
    const int ur = 16 * w + 4 * kq + reg;
    in[reg] = u0 + 4 * kq + reg < a.nq;
    lo[reg] = goff[ur];
    int l = 0, h = goff[ur + 1] - lo[reg];
    while (l < h) {
      const int m = (l + h) >> 1;
      if (gk[lo[reg] + m] != PKEY_MAX) l = m + 1; else h = m;
    }
    nv[reg] = l;
    thr[reg] = l > 0 ? gk[lo[reg] + l - 1] : 0ull;
    thrf[reg] = l > 0 ? -topn_key_score((uint32_t)(thr[reg] >> 32)) : __builtin_inff();
  }
  S sc{ka.m};
  rank_stream<KS, VEC>(a, sc, sc, smem, u0, in, i_lo, i_hi, a.n, [&](const v4& acc, const v4* slot, int64_t cand) __attribute__((always_inline)) {
    const auto spare = sc.staged(slot);
    const bool iok = cand < i_hi && sc.live(spare);
#pragma unroll
    for (int reg = 0; reg < 4; ++reg) {
      const float s = sc.score(acc[reg], reg, spare);
      const bool above = s > thrf[reg], maybe = !(s < thrf[reg]) && iok;
      if (!__builtin_amdgcn_ballot_w64(maybe)) continue;                   // most 64-score slots leave here
      const uint64_t key = topn_key(s, true, (uint32_t)cand);
      bool c = maybe && (above || key < thr[reg]) && nv[reg] > 0;
      if (c && a.bm) c = ((a.bm[(u0 + 4 * kq + reg) * a.bm_words + (cand >> 5)] >> (cand & 31)) & 1u) == 0u;
      if (c) {
        const uint64_t* keys = gk + lo[reg];
        int l = 0, h = nv[reg] - 1;                                        // the first gold key that is not before this one (the worst is not)
        while (l < h) {
          const int m = (l + h) >> 1;
          if (keys[m] < key) l = m + 1; else h = m;
        }
        if (keys[l] != key) atomicAdd(cnt + lo[reg] + l, 1u);              // (the same key is the same candidate: the gold itself)
      }
    }
  });
  // (behind the stream's last barrier)  One thread per user: the running sum over its buckets is the split's share of each rank
  if (tid < 64) {
    const int l0 = goff[tid], l1 = goff[tid + 1];
    uint32_t run = 0u;
    for (int p = l0; p < l1; ++p) {
      if (gk[p] == PKEY_MAX) break;
      run += cnt[p];
      if (run) atomicAdd(a.ranks + g_lo + a.perm[g_lo + p], (int32_t)run);
    }
  }
}

template <class S, int KS, class MA>
int launch_rank(const MA& m, const RankArgs& r, bool vec, hipStream_t st, const char* name) {
  static_assert(SweepGeom<KS>::STAGES + S::LDS + rank_gold_lds(rank_cap(KS)) <= SWEEP_LDS_MAX, "the stages, what the scorer holds and the gold keys fit the LDS");
  const size_t lds = SweepGeom<KS>::STAGES + S::LDS + rank_gold_lds(r.gcap);
  const RankKernelArgs<MA> ka{m, r};
  const unsigned nub = (unsigned)((r.nq + 63) / 64);
  auto go = [&](void (*keys)(RankKernelArgs<MA>), void (*count)(RankKernelArgs<MA>)) {
    (void)hipFuncSetAttribute((const void*)keys, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    (void)hipFuncSetAttribute((const void*)count, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    hipLaunchKernelGGL(keys, dim3(nub), dim3(256), lds, st, ka);
    if (int rc = check_launch(name)) return rc;
    hipLaunchKernelGGL(count, dim3(nub * (unsigned)r.nsplit), dim3(256), lds, st, ka);
    return check_launch(name);
  };
  return vec ? go(rank_keys_kernel<S, KS, true, MA>, rank_count_kernel<S, KS, true, MA>)
             : go(rank_keys_kernel<S, KS, false, MA>, rank_count_kernel<S, KS, false, MA>);
}

bool rank_shape_ok(int d, int64_t n, int64_t block_golds) {
  return d >= 1 && d <= 256 && n > 0 && n < ((int64_t)1 << 31) && block_golds >= 0 && block_golds <= rank_cap_d(d);
}

// workspace: the sorted keys (8-byte entries) | their permutation (padded to 8 bytes) | the filter bits | cand_floats floats per candidate
size_t rank_perm_bytes(int64_t n_gold) { return ((size_t)n_gold * sizeof(int32_t) + 7) / 8 * 8; }
size_t rank_workspace_bytes(int d, int64_t nq, int64_t n, int64_t n_gold, int64_t block_golds, int cand_floats) {
  if (nq <= 0 || n_gold <= 0 || !rank_shape_ok(d, n, block_golds)) return 0;
  return (size_t)n_gold * sizeof(uint64_t) + rank_perm_bytes(n_gold) + (size_t)nq * (size_t)((n + 31) / 32) * sizeof(uint32_t) +
         (size_t)cand_floats * n * sizeof(float) + 16;
}

// What both entry points check and set up: the argument rules, the declines, the workspace and the filter bits.  *done: nothing to launch.
int rank_prepare(const char* name, RankArgs& r, int d, const int64_t* u_ids, int64_t nq, int64_t n, const int64_t* filt_off, const int32_t* filt_ids,
                 const int64_t* gold_off, const int32_t* gold_ids, int64_t n_gold, int64_t block_golds, int nsplit, int32_t* ranks, void* ws,
                 float** cand_floats, hipStream_t st, bool* done) {
  *done = true;
  KTUP_REQUIRE(nq >= 0 && n_gold >= 0 && nsplit >= 0 && block_golds >= 0, "%s: bad sizes (%lld users, n_gold %lld, block_golds %lld, nsplit %d)", name,
               (long long)nq, (long long)n_gold, (long long)block_golds, nsplit);
  KTUP_REQUIRE((filt_off == nullptr) == (filt_ids == nullptr), "%s: filt_off and filt_ids go together", name);
  KTUP_REQUIRE(gold_off, "%s: null gold_off", name);
  KTUP_REQUIRE(gold_ids || n_gold == 0, "%s: gold_off without gold_ids (n_gold %lld)", name, (long long)n_gold);
  KTUP_REQUIRE(ranks || n_gold == 0, "%s: null ranks", name);
  KTUP_REQUIRE(block_golds <= n_gold, "%s: block_golds %lld above n_gold %lld", name, (long long)block_golds, (long long)n_gold);
  if (d > 256) return set_error(KTUP_ERR_UNSUPPORTED, "%s: embedding_size %d > 256", name, d);
  if (n >= ((int64_t)1 << 31)) return set_error(KTUP_ERR_UNSUPPORTED, "%s: %lld candidates do not fit 32-bit ids", name, (long long)n);
  if (block_golds > rank_cap_d(d))
    return set_error(KTUP_ERR_UNSUPPORTED, "%s: a 64-user block with %lld gold entries (at most %d at embedding_size %d)", name, (long long)block_golds,
                     rank_cap_d(d), d);
  if (nq == 0 || n_gold == 0) return KTUP_OK;
  KTUP_REQUIRE(u_ids && ws, "%s: null id or workspace pointer", name);
  KTUP_REQUIRE((reinterpret_cast<uintptr_t>(ws) & 15) == 0, "%s: the workspace must be 16-byte aligned", name);
  r.u_ids = u_ids; r.nq = nq; r.n = n; r.d = d;
  r.gold_off = gold_off; r.gold_ids = gold_ids; r.ranks = ranks;
  r.gcap = (int)((block_golds + 63) / 64 * 64);
  if (r.gcap < 64) r.gcap = 64;
  r.nsplit = sweep_nsplit(nq, n, TOPN_MAX, nsplit, &r.split);
  if ((nq + 63) / 64 * r.nsplit > 0x7fffffffLL) return set_error(KTUP_ERR_UNSUPPORTED, "%s: too many users for one call (%lld)", name, (long long)nq);
  r.skey = reinterpret_cast<uint64_t*>(ws);
  r.perm = reinterpret_cast<int32_t*>(r.skey + n_gold);
  uint32_t* bm = reinterpret_cast<uint32_t*>(reinterpret_cast<char*>(r.perm) + rank_perm_bytes(n_gold));
  r.bm = nullptr;
  r.bm_words = (n + 31) / 32;
  if (cand_floats) *cand_floats = reinterpret_cast<float*>(bm + nq * r.bm_words);
  if (filt_off) {
    if (int rc = sweep_filter_bits(filt_off, filt_ids, nq, n, bm, r.bm_words, st, name)) return rc;
    r.bm = bm;
  }
  *done = false;
  return KTUP_OK;
}

}  // namespace
}  // namespace ktup

using namespace ktup;

extern "C" int ktup_eval_dot_ranks_supported(int d, int64_t n_items, int64_t block_golds) { return rank_shape_ok(d, n_items, block_golds) ? 1 : 0; }

extern "C" size_t ktup_eval_dot_ranks_workspace_bytes(int d, int64_t nq, int64_t n_items, int64_t n_gold, int64_t block_golds) {
  return rank_workspace_bytes(d, nq, n_items, n_gold, block_golds, 0);
}

extern "C" int ktup_eval_dot_ranks(const float* U, int64_t ldu, const float* I, int64_t ldi, int d, const int64_t* u_ids, int64_t nq,
                                   int64_t n_items, const float* user_add, const float* item_add, const int64_t* filt_off,
                                   const int32_t* filt_ids, const int64_t* gold_off, const int32_t* gold_ids, int64_t n_gold,
                                   int64_t block_golds, int nsplit, int32_t* ranks, void* ws, void* stream) {
  const char* name = "ktup_eval_dot_ranks";
  KTUP_REQUIRE(U && I, "%s: null table pointer", name);
  KTUP_REQUIRE(d >= 1 && n_items > 0, "%s: bad sizes (embedding_size %d, %lld items)", name, d, (long long)n_items);
  KTUP_REQUIRE(ldu >= d && ldi >= d, "%s: a row pitch is below embedding_size %d", name, d);
  hipStream_t st = (hipStream_t)stream;
  RankArgs r{};
  bool done;
  if (int rc = rank_prepare(name, r, d, u_ids, nq, n_items, filt_off, filt_ids, gold_off, gold_ids, n_gold, block_golds, nsplit, ranks, ws, nullptr, st,
                            &done))
    return rc;
  if (done) return KTUP_OK;
  DotArgs a{};
  a.U = U; a.ldu = ldu; a.I = I; a.ldi = ldi; a.user_add = user_add; a.item_add = item_add;
  const bool vec = d % 4 == 0 && ldi % 4 == 0 && (reinterpret_cast<uintptr_t>(I) & 15) == 0;
  return with_k_steps(d, [&](auto ks) {
    constexpr int KS = decltype(ks)::value;
    return launch_rank<DotScorer<KS>, KS>(a, r, vec, st, name);
  });
}

extern "C" int ktup_eval_cfkg_ranks_supported(int d, int64_t n_cand, int64_t block_golds) { return rank_shape_ok(d, n_cand, block_golds) ? 1 : 0; }

extern "C" size_t ktup_eval_cfkg_ranks_workspace_bytes(int d, int64_t nq, int64_t n_cand, int64_t n_gold, int64_t block_golds) {
  return rank_workspace_bytes(d, nq, n_cand, n_gold, block_golds, 1);
}

extern "C" int ktup_eval_cfkg_ranks(const float* U, int64_t ldu, const float* R, int64_t ldr, int64_t rel, const float* E, int64_t lde,
                                    int64_t n_ent, const int64_t* cand_ids, int64_t n_cand, int d, const int64_t* u_ids, int64_t nq, int l1,
                                    const int64_t* filt_off, const int32_t* filt_ids, const int64_t* gold_off, const int32_t* gold_ids,
                                    int64_t n_gold, int64_t block_golds, int nsplit, int32_t* ranks, void* ws, void* stream) {
  const char* name = "ktup_eval_cfkg_ranks";
  KTUP_REQUIRE(U && R && E, "%s: null table pointer", name);
  KTUP_REQUIRE(d >= 1 && n_ent > 0 && n_cand > 0, "%s: bad sizes (embedding_size %d, %lld entities, %lld candidates)", name, d, (long long)n_ent,
               (long long)n_cand);
  KTUP_REQUIRE(ldu >= d && ldr >= d && lde >= d, "%s: a row pitch is below embedding_size %d", name, d);
  KTUP_REQUIRE(rel >= 0, "%s: negative relation row (got %lld)", name, (long long)rel);
  KTUP_REQUIRE(cand_ids || n_cand == n_ent, "%s: without cand_ids the candidates are the %lld entity rows (got n_cand %lld)", name,
               (long long)n_ent, (long long)n_cand);
  hipStream_t st = (hipStream_t)stream;
  RankArgs r{};
  bool done;
  float* en = nullptr;
  if (int rc = rank_prepare(name, r, d, u_ids, nq, n_cand, filt_off, filt_ids, gold_off, gold_ids, n_gold, block_golds, nsplit, ranks, ws, &en, st, &done))
    return rc;
  if (done) return KTUP_OK;
  CfkgPassArgs a{};
  a.U = U; a.ldu = ldu; a.R = R; a.ldr = ldr; a.rel = rel; a.E = E; a.lde = lde; a.n_ent = n_ent; a.cand_ids = cand_ids; a.enorm = nullptr;
  if (!l1) {
    hipLaunchKernelGGL(cfkg_cand_norm_kernel, dim3((unsigned)min((n_cand + 15) / 16, (int64_t)4096)), dim3(256), 0, st, E, lde, n_ent, cand_ids,
                       n_cand, d, en);
    if (int rc = check_launch(name)) return rc;
    a.enorm = en;
  }
  const bool vec = d % 4 == 0 && lde % 4 == 0 && (reinterpret_cast<uintptr_t>(E) & 15) == 0;
  return with_k_steps(d, [&](auto ks) {
    constexpr int KS = decltype(ks)::value;
    return l1 ? launch_rank<CfkgScorer<KS, true>, KS>(a, r, vec, st, name) : launch_rank<CfkgScorer<KS, false>, KS>(a, r, vec, st, name);
  });
}
