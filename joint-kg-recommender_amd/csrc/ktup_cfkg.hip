// The rec step of CFKG (CFKG.py:66-80: user + buy - item-entity, the BPR loss of knowledgable_recommendation.py:335-344) in ONE
// launch -- see include/ktup_hip.h.
//
// cfkg_rec_step_kernel: a gather and scatter of four rows per example, shaped as dot_step_kernel (ktup_dot_step.hip).  One wave64
// owns an example (four in flight per workgroup): it reads the user row, the relation row and the positive and negative entity rows
// ONCE, reduces the two distances across its lanes, evaluates the BPR term and its derivative on every lane and adds the user row
// and the two entity rows with float atomics.  The relation row is the one address every pair of the batch hits: a wave keeps its
// share of that gradient in registers across the examples it walks, the workgroup's four waves sum through LDS, and each workgroup
// issues ONE row add with contiguous lanes (at most 256 workgroups are launched, whatever B).  The loss partial leaves the same way.
//
// cfkg_pass_kernel: the whole rec evaluation pass (CFKG.py:100-118 + the filtered top-n of utils/misc.py:186-248) in one sweep that
// never writes the (users x candidates) matrix, structured as dot_pass_kernel (ktup_dot_pass.hip): a workgroup owns 64 users
// (4 waves x 16) and a contiguous split of the candidates; the users' query rows c = U[u] + R[rel] are formed once and held for the
// pass; candidate rows (gathered through cand_ids) stream through a double-buffered LDS stage whose next contents are in flight under
// this stage's arithmetic; filter lists are bits, built once per pass; candidates go through pending rows into a sorted list per
// user (ktup_topn.h), and the splits' lists are merged by topk_merge_kernel.
//   * squared L2: |c|^2 - 2 c.e + |e|^2 with c.e on v_mfma_f32_16x16x4_f32 (the c rows in registers, one float per lane and 4 k);
//     |e|^2 is computed once per pass (cfkg_cand_norm_kernel) and rides in the staged row's spare slot;
//   * L1: on the VALU against the same stage, the wave's 16 query rows in LDS; every lane owns the 4 users x 16-candidate-tile
//     slots the MFMA would have given it, so the ranking code is one.
// The spare slot also carries whether the candidate's entity row exists: a cand_ids entry outside [0, n_ent) is never ranked and
// never dereferenced (the stage reads row 0 in its place).
#include <hip/hip_runtime.h>

#include <cstdint>

#include "ktup_lane_swap.h"
#include "ktup_rows.h"
#include "ktup_topn.h"

using namespace ktup;

namespace {

constexpr int MAX_D = 256;
constexpr int MAX_BLOCKS = 256;  // one relation-row add per workgroup: at most one per CU

// -log(sigmoid(x)) the way torch's logsigmoid evaluates it (ktup_loss.hip pair_loss_fused_kernel)
KTUP_DEV float neg_logsigmoid(float x) { return fmaxf(-x, 0.f) + log1pf(expf(-fabsf(x))); }
KTUP_DEV float sigmoidf(float x) { return 1.f / (1.f + expf(-x)); }

KTUP_DEV void put_cols(float* row, int c, float v) { row[c] = v; }
KTUP_DEV void put_cols(float* row, int c, float4 v) { row[4 * c] = v.x; row[4 * c + 1] = v.y; row[4 * c + 2] = v.z; row[4 * c + 3] = v.w; }

struct CfkgStepArgs {
  const float *U, *E, *R;
  int64_t ldu, lde, ldr, rel;
  const int64_t *u_ids, *i_ids;
  int64_t B;
  int d, l1;
  float target, up;
  float* loss;
  float *gU, *gE, *gR;
  int nch;  // chunks of V per row
};

template <typename V, int CPL>
__global__ __launch_bounds__(256) void cfkg_rec_step_kernel(CfkgStepArgs a) {
  __shared__ float red[4];
  __shared__ float rsum[4][MAX_D];                                  // the waves' relation-row gradients, by column
  const RowCtx<V, 64, CPL> cx{a.nch, (int)(threadIdx.x & 63)};
  const int wave = threadIdx.x >> 6;
  const bool l1 = a.l1 != 0;
  const float gmean = a.up / (float)a.B;
  V rr[CPL], gr[CPL];
  cx.load(rr, a.R + a.rel * a.ldr);
#pragma unroll
  for (int j = 0; j < CPL; ++j) vzero(gr[j]);
  float part = 0.f;
  for (int64_t k = (int64_t)blockIdx.x * 4 + wave; k < a.B; k += (int64_t)gridDim.x * 4) {
    const int64_t u = a.u_ids[k], ip = a.i_ids[k], in = a.i_ids[a.B + k];
    V c[CPL], zp[CPL], zn[CPL];
    cx.load(c, a.U + u * a.ldu);
    cx.load(zp, a.E + ip * a.lde);
    cx.load(zn, a.E + in * a.lde);
    float sp = 0.f, sn = 0.f;
#pragma unroll
    for (int j = 0; j < CPL; ++j) {                                 // (columns past the width hold zeros: distance and derivative 0)
      c[j] = vadd(c[j], rr[j]);
      zp[j] = vsub(c[j], zp[j]);
      zn[j] = vsub(c[j], zn[j]);
      sp += vdist(zp[j], l1);
      sn += vdist(zn[j], l1);
    }
    sp = group_sum<64>(sp);
    sn = group_sum<64>(sn);
    const float x = a.target * (sp - sn);
    part += neg_logsigmoid(x);                                      // (the same value on every lane; lane 0's is used)
    const float g = -gmean * a.target * sigmoidf(-x);               // d/d s_pos; -g is d/d s_neg
    V gu[CPL], gp[CPL], gn[CPL];
#pragma unroll
    for (int j = 0; j < CPL; ++j) {
      const V vp = vddist(zp[j], l1), vn = vddist(zn[j], l1);
      gu[j] = vscale(g, vsub(vp, vn));
      gp[j] = vscale(-g, vp);
      gn[j] = vscale(g, vn);
      gr[j] = vadd(gr[j], gu[j]);
    }
    cx.scatter_add(a.gU + u * a.ldu, gu);
    cx.scatter_add(a.gE + ip * a.lde, gp);
    cx.scatter_add(a.gE + in * a.lde, gn);
  }
#pragma unroll
  for (int j = 0; j < CPL; ++j) {
    const int ch = cx.lane + j * 64;
    if (ch < a.nch) put_cols(rsum[wave], ch, gr[j]);
  }
  if (cx.lane == 0) red[wave] = part;
  __syncthreads();
  const int t = threadIdx.x;
  if (t < a.d) {                                                    // one row add per workgroup, thread t on column t
    const float s = (rsum[0][t] + rsum[1][t]) + (rsum[2][t] + rsum[3][t]);
    if (s != 0.f) atomicAdd(a.gR + a.rel * a.ldr + t, s);
  }
  if (t == 0) {
    const float total = (red[0] + red[1]) + (red[2] + red[3]);
    if (total != 0.f) atomicAdd(a.loss, total * gmean);
  }
}

}  // namespace

extern "C" int ktup_train_cfkg_rec_step_supported(int d) { return (d >= 1 && d <= MAX_D && !opt_deterministic()) ? 1 : 0; }

extern "C" int ktup_train_cfkg_rec_step(const float* U, int64_t ldu, const float* E, int64_t lde, const float* R, int64_t ldr, int64_t rel,
                                        int d, const int64_t* u_ids, const int64_t* i_ids, int64_t B, int l1, float target, float up,
                                        float* loss, float* gU, float* gE, float* gR, void* stream) {
  const char* name = "ktup_train_cfkg_rec_step";
  KTUP_REQUIRE(d >= 1, "%s: embedding_size must be positive (got %d)", name, d);
  KTUP_REQUIRE(B >= 1, "%s: the batch needs at least one example (got %lld)", name, (long long)B);
  KTUP_REQUIRE(U && E && R && u_ids && i_ids && loss && gU && gE && gR, "%s: null pointer argument", name);
  KTUP_REQUIRE(ldu >= d && lde >= d && ldr >= d, "%s: a row pitch below the width", name);
  KTUP_REQUIRE(rel >= 0, "%s: negative relation row (got %lld)", name, (long long)rel);
  if (d > MAX_D) return set_error(KTUP_ERR_UNSUPPORTED, "%s: embedding_size %d is beyond the %d columns a wave holds", name, d, MAX_D);
  if (opt_deterministic())
    return set_error(KTUP_ERR_UNSUPPORTED, "%s: the row gradients are float atomics of many workgroups (option deterministic is set)", name);
  CfkgStepArgs a{U, E, R, ldu, lde, ldr, rel, u_ids, i_ids, B, d, l1, target, up, loss, gU, gE, gR, 0};
  const bool vec = can_vec4(d, {U, E, R, gU, gE, gR}, {ldu, lde, ldr});
  const int grid = grid_for((B + 3) / 4, MAX_BLOCKS);
  hipStream_t st = (hipStream_t)stream;
  if (vec) {
    a.nch = d / 4;                                                  // <= 64: one float4 per lane
    hipLaunchKernelGGL((cfkg_rec_step_kernel<float4, 1>), dim3(grid), dim3(256), 0, st, a);
  } else {
    a.nch = d;
    if (d <= 64) hipLaunchKernelGGL((cfkg_rec_step_kernel<float, 1>), dim3(grid), dim3(256), 0, st, a);
    else if (d <= 128) hipLaunchKernelGGL((cfkg_rec_step_kernel<float, 2>), dim3(grid), dim3(256), 0, st, a);
    else hipLaunchKernelGGL((cfkg_rec_step_kernel<float, 4>), dim3(grid), dim3(256), 0, st, a);
  }
  return check_launch(name);
}

// ================================================================================================ the evaluation pass
namespace ktup {
namespace {

constexpr int NSPLIT_MAX = 32;   // candidate splits: NSPLIT_MAX * TOPN_MAX keys per user is what the merge holds, eight per lane
constexpr int MERGE_PER_LANE = NSPLIT_MAX * TOPN_MAX / 64;
constexpr size_t WAVE_LDS = (size_t)16 * PCAP * 8 + (size_t)16 * 16 * 8;   // pending rows | lists

// The filter lists of a pass as bits, once per pass: bm[b * words + (j >> 5)] bit (j & 31), one wave per user of u_ids.
__global__ __launch_bounds__(256) void cfkg_filter_zero_kernel(uint32_t* __restrict__ bm, int64_t n) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) bm[i] = 0u;
}
__global__ __launch_bounds__(256) void cfkg_filter_bits_kernel(const int64_t* __restrict__ off, const int32_t* __restrict__ ids, int64_t nq,
                                                               int64_t n_cand, uint32_t* __restrict__ bm, int64_t words) {
  const int lane = threadIdx.x & 63;
  for (int64_t b = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); b < nq; b += (int64_t)gridDim.x * 4) {
    const int64_t f1 = off[b + 1];
    for (int64_t f = off[b] + lane; f < f1; f += 64) {
      const int64_t id = ids[f];
      if (id >= 0 && id < n_cand) atomicOr(bm + b * words + (id >> 5), 1u << (id & 31));
    }
  }
}

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

struct CfkgPassArgs {
  const float* U; int64_t ldu;
  const float* R; int64_t ldr, rel;
  const float* E; int64_t lde, n_ent;
  const int64_t* cand_ids;              // NULL: candidate j is row j
  const float* enorm;                   // [n_cand] |e|^2 (squared L2); NULL under L1
  int d, evec;                          // evec: entity rows are whole, 16-byte aligned float4 (else element by element)
  const int64_t* u_ids; int64_t nq, n_cand;
  const uint32_t* bm; int64_t bm_words; // the filter bits [nq][bm_words]; NULL = no filter
  int topn, nsplit; int64_t split_items;
  uint64_t* part;                       // [nq][nsplit][topn] partial lists
};

// KS: 4-wide k steps (d <= 4 KS; the padding holds zeros on both sides: it adds nothing to a dot product or to a distance)
template <int KS, bool L1>
struct CfkgGeom {
  static constexpr int ST = KS > 32 ? 32 : 64;       // candidates per stage
  static constexpr int NSUB = ST / 16;               // 16-candidate tiles per stage = accumulators per wave
  static constexpr int CPR = KS + 1;                 // float4 slots per row: KS operand quads + {|e|^2, row exists, 0, 0}
  static constexpr int ROW4 = CPR | 1;               // the row's float4 pitch in LDS: odd
  static constexpr int STG = ST * ROW4;              // float4 per stage buffer
  static constexpr int SLOTS = ST * KS;              // operand quads a stage loads
  static constexpr int NPRE = (SLOTS + 255) / 256;   // float4 per thread in flight for the next stage
  static constexpr int CROW4 = KS | 1;               // L1: float4 pitch of a query row in LDS
  static constexpr size_t CW = L1 ? (size_t)16 * CROW4 * 16 : 0;   // L1: a wave's 16 query rows
  static constexpr size_t LDS = (size_t)2 * STG * 16 + 4 * CW + 4 * WAVE_LDS;
};

template <int KS, bool VEC, bool L1>
__global__ __launch_bounds__(256, 2) void cfkg_pass_kernel(CfkgPassArgs a) {
  using G = CfkgGeom<KS, L1>;
  constexpr int ST = G::ST, NSUB = G::NSUB, ROW4 = G::ROW4, STG = G::STG, SLOTS = G::SLOTS, NPRE = G::NPRE, CROW4 = G::CROW4;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  v4* Xb = reinterpret_cast<v4*>(smem);                                   // [2][STG] candidate stages
  const int tid = threadIdx.x, lane = tid & 63, kq = lane >> 4, j = lane & 15;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  float* cwf = reinterpret_cast<float*>(smem + (size_t)2 * STG * 16 + (size_t)w * G::CW);   // L1: [16][CROW4] float4, this wave's query rows
  uint64_t* pbuf = reinterpret_cast<uint64_t*>(smem + (size_t)2 * STG * 16 + 4 * G::CW + (size_t)w * WAVE_LDS);   // [16][PCAP] pending candidates
  uint64_t* tk = pbuf + 16 * PCAP;                                        // [16][16] the users' sorted lists (touched by merges only)
  const int64_t ub = (int64_t)(blockIdx.x / (unsigned)a.nsplit);
  const int sp = (int)(blockIdx.x - (unsigned)ub * (unsigned)a.nsplit);
  const int64_t u0 = ub * 64 + 16 * w;
  const int64_t i_lo = (int64_t)sp * a.split_items;
  const int64_t i_hi = min(a.n_cand, i_lo + a.split_items);
  const int topn = a.topn, d = a.d;
  for (int idx = lane; idx < 16 * 16; idx += 64) tk[idx] = PKEY_MAX;
  // The query rows of the whole pass: lane (kq, j) forms c[user j][4 s + kq] = U[u][.] + R[rel][.] for every k step s
  float av[KS];
  {
    const bool ok = u0 + j < a.nq;
    const float* urow = a.U + (ok ? a.u_ids[u0 + j] : 0) * a.ldu;
    const float* rrow = a.R + a.rel * a.ldr;
#pragma unroll
    for (int s = 0; s < KS; ++s) {                                         // (unconditional, from clamped addresses: all in flight together)
      const int kk = min(4 * s + kq, d - 1);
      av[s] = urow[kk] + rrow[kk];
    }
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int s = 0; s < KS; ++s) av[s] = (ok && 4 * s + kq < d) ? av[s] : 0.f;
  }
  float cn[4] = {0.f, 0.f, 0.f, 0.f};                                     // squared L2: |c|^2 of the users of this lane's accumulator rows
  if constexpr (L1) {
#pragma unroll
    for (int s = 0; s < KS; ++s) cwf[(j * CROW4 + s) * 4 + kq] = av[s];   // (read after the workgroup barrier below)
  } else {
    float cnj = 0.f;
#pragma unroll
    for (int s = 0; s < KS; ++s) cnj = fmaf(av[s], av[s], cnj);
    cnj += __shfl_xor(cnj, 16, 64);
    cnj += __shfl_xor(cnj, 32, 64);                                       // |c|^2 of user j on every lane (., j)
#pragma unroll
    for (int reg = 0; reg < 4; ++reg) cn[reg] = __shfl(cnj, 4 * kq + reg, 64);
  }
  uint64_t thr[4];                                                        // the users' n-th keys (rows past the end: nothing is ever below)
  // ... and their NEGATED scores (the sweep ranks s = -distance descending, like the inner-product pass: a value above is a candidate,
  // one below is not -- one float compare per score; an equal one, a NaN on either side (the threshold of a list that is still
  // short is one) or a zero of the other sign goes through the 64-bit key compare, so the order is that of the keys in every case)
  float thrf[4];
  int pend[4] = {0, 0, 0, 0};
#pragma unroll
  for (int reg = 0; reg < 4; ++reg) {
    const int64_t ur = u0 + 4 * kq + reg;
    thr[reg] = ur < a.nq ? PKEY_MAX : 0ull;
    thrf[reg] = ur < a.nq ? __uint_as_float(0x7fffffffu) : __builtin_inff();
  }
  // ---- the stage loads: slot e of a stage = operand quad c of candidate r (r = e / KS); candidates past the end re-read the last
  // one, candidates without an entity row read row 0 (both are masked out below, the operands only have to be there).  Straight-line
  // code: every load is unconditional from a clamped address, so that all loads of a stage are in flight together.
  v4 pre[NPRE];
  float pre_add = 0.f, pre_ok = 0.f;
  auto cand_row = [&](int64_t c, bool& ok) __attribute__((always_inline)) {
    const int64_t id = a.cand_ids ? a.cand_ids[c] : c;
    ok = id >= 0 && id < a.n_ent;
    return ok ? id : (int64_t)0;
  };
  auto fetch = [&](int64_t row0) __attribute__((always_inline)) {
#pragma unroll
    for (int k = 0; k < NPRE; ++k) {
      const int e = min(tid + 256 * k, SLOTS - 1);
      const int r = e / KS, c = e - r * KS;
      bool ok;
      const float* row = a.E + cand_row(min(row0 + r, a.n_cand - 1), ok) * a.lde;
      if constexpr (VEC) {
        pre[k] = *reinterpret_cast<const v4*>(row + min(4 * c, d - 4));
      } else {
#pragma unroll
        for (int q = 0; q < 4; ++q) pre[k][q] = row[min(4 * c + q, d - 1)];
      }
    }
    const int64_t mine = min(row0 + min(tid, ST - 1), a.n_cand - 1);
    bool ok;
    (void)cand_row(mine, ok);
    pre_ok = ok ? 1.f : 0.f;
    if (a.enorm) pre_add = a.enorm[mine];
  };
  auto stash = [&](int buf) __attribute__((always_inline)) {
#pragma unroll
    for (int k = 0; k < NPRE; ++k) {
      const int e = tid + 256 * k;
      if (e >= SLOTS) continue;
      const int r = e / KS, c = e - r * KS;
      v4 v = pre[k];                                                       // (the padding is zeroed here, not at the load)
      if (d != 4 * KS) {
#pragma unroll
        for (int q = 0; q < 4; ++q) v[q] = 4 * c + q < d ? v[q] : 0.f;
      }
      Xb[buf * STG + r * ROW4 + c] = v;
    }
    if (tid < ST) Xb[buf * STG + tid * ROW4 + KS] = (v4){pre_add, pre_ok, 0.f, 0.f};
  };
  // ---- ranking (see ktup_dot_pass.hip): candidates are appended to the user's pending row in LDS at positions taken from a ballot
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
        thrf[reg] = -topn_key_score(nhi);                                               // negated (NaN: list short)
      }
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
  };
  // 16 users x the 16 candidates [cand - j, cand - j + 16): acc holds c.e (squared L2) or the distance itself (L1)
  auto rank_tile = [&](const v4& acc, float en, bool exists, int64_t cand) __attribute__((always_inline)) {
    const bool iok = cand < i_hi && exists;
    bool full = false;
#pragma unroll
    for (int reg = 0; reg < 4; ++reg) {
      const int ur = 4 * kq + reg;
      const float dist = L1 ? acc[reg] : __fadd_rn(fmaf(-2.f, acc[reg], cn[reg]), en);
      const float s = -dist;
      const bool above = s > thrf[reg], maybe = !(s < thrf[reg]) && iok;
      if (!__builtin_amdgcn_ballot_w64(maybe)) continue;                   // most 64-score slots leave here
      const uint64_t key = topn_key(s, true, (uint32_t)cand);              // (negated back: ascending distance, ties -> lower j)
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
    if constexpr (L1) {
      const v4* cw = reinterpret_cast<const v4*>(cwf) + 4 * kq * CROW4;    // the four users of this lane's accumulator rows
#pragma unroll 2
      for (int s = 0; s < KS; ++s) {
        v4 cq[4];
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) cq[reg] = cw[reg * CROW4 + s];
#pragma unroll
        for (int t = 0; t < NSUB; ++t) {
          const v4 e = eb[t * 16 * ROW4 + s];
#pragma unroll
          for (int reg = 0; reg < 4; ++reg) {
            const v4 z = cq[reg] - e;
            acc[t][reg] += (fabsf(z[0]) + fabsf(z[1])) + (fabsf(z[2]) + fabsf(z[3]));
          }
        }
      }
    } else {
      const float* rb = reinterpret_cast<const float*>(eb) + kq;           // lane (kq, candidate j): element kq of every k quad
#pragma unroll
      for (int s = 0; s < KS; ++s) {
#pragma unroll
        for (int t = 0; t < NSUB; ++t) acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[s], rb[t * 16 * ROW4 * 4 + 4 * s], acc[t], 0, 0, 0);
      }
    }
#pragma unroll
    for (int t = 0; t < NSUB; ++t) {
      if (row0 + 16 * t >= i_hi) break;                                    // (uniform)
      const v4 spare = eb[t * 16 * ROW4 + KS];
      rank_tile(acc[t], spare[0], spare[1] != 0.f, row0 + 16 * t + j);
    }
  };
  const int64_t nst = (i_hi - i_lo + ST - 1) / ST;
  fetch(i_lo);
  stash(0);
  __syncthreads();                                                         // stage 0, the query rows (L1) and the lists are in place
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
  if (j < topn) {
#pragma unroll
    for (int reg = 0; reg < 4; ++reg) {
      const int64_t ur = u0 + 4 * kq + reg;
      if (ur < a.nq) a.part[(ur * a.nsplit + sp) * topn + j] = tk[(4 * kq + reg) * 16 + j];
    }
  }
}

template <int KS, bool VEC, bool L1>
int launch_cfkg_pass_one(const CfkgPassArgs& a, unsigned blocks, hipStream_t st, const char* name) {
  constexpr size_t lds = CfkgGeom<KS, L1>::LDS;
  static_assert(lds <= 160 * 1024, "the stages, the query rows and the lists fit the LDS");
  (void)hipFuncSetAttribute((const void*)cfkg_pass_kernel<KS, VEC, L1>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  hipLaunchKernelGGL((cfkg_pass_kernel<KS, VEC, L1>), dim3(blocks), dim3(256), lds, st, a);
  return check_launch(name);
}

template <int KS>
int launch_cfkg_pass(const CfkgPassArgs& a, bool l1, unsigned blocks, hipStream_t st, const char* name) {
  if (l1) return a.evec ? launch_cfkg_pass_one<KS, true, true>(a, blocks, st, name) : launch_cfkg_pass_one<KS, false, true>(a, blocks, st, name);
  return a.evec ? launch_cfkg_pass_one<KS, true, false>(a, blocks, st, name) : launch_cfkg_pass_one<KS, false, false>(a, blocks, st, name);
}

// how the candidates are cut: `want` splits, whole 16-candidate tiles each; 0: about 1.25 workgroups per CU (the rule and the
// measurements of ktup_dot_pass.hip's dot_nsplit).
int cfkg_nsplit(int64_t nq, int64_t n_cand, int want, int64_t* split_items) {
  const int64_t nub = (nq + 63) / 64;
  int64_t ns = want > 0 ? want : (320 + nub - 1) / (nub > 0 ? nub : 1);
  ns = ns < 1 ? 1 : ns > NSPLIT_MAX ? NSPLIT_MAX : ns;
  int64_t si = (n_cand + ns - 1) / ns;
  si = (si + 15) / 16 * 16;
  if (want <= 0 && si < 256) si = 256;                                     // (a workgroup's prologue wants some candidates to pay for it)
  *split_items = si;
  return (int)((n_cand + si - 1) / si);
}

}  // namespace
}  // namespace ktup

extern "C" size_t ktup_eval_cfkg_topk_workspace_bytes(int d, int64_t nq, int64_t n_cand, int topn, int nsplit) {
  (void)d;
  if (nq <= 0 || n_cand <= 0 || topn <= 0 || topn > TOPN_MAX || nsplit < 0) return 0;
  int64_t si = 0;
  const int ns = cfkg_nsplit(nq, n_cand, nsplit, &si);
  const size_t part = (size_t)nq * ns * topn * sizeof(uint64_t);
  const size_t bits = (size_t)nq * (size_t)((n_cand + 31) / 32) * sizeof(uint32_t);
  return part + bits + (size_t)n_cand * sizeof(float) + 16;
}

extern "C" int ktup_eval_cfkg_topk(const float* U, int64_t ldu, const float* R, int64_t ldr, int64_t rel, const float* E, int64_t lde,
                                   int64_t n_ent, const int64_t* cand_ids, int64_t n_cand, int d, const int64_t* u_ids, int64_t nq, int l1,
                                   const int64_t* filt_off, const int32_t* filt_ids, int topn, int nsplit, int32_t* top_ids,
                                   float* top_scores, void* ws, void* stream) {
  const char* name = "ktup_eval_cfkg_topk";
  KTUP_REQUIRE(U && R && E && u_ids && top_ids && ws, "%s: null table, id, output or workspace pointer", name);
  KTUP_REQUIRE(d >= 1 && nq >= 0 && n_ent > 0 && n_cand > 0 && topn > 0 && nsplit >= 0,
               "%s: bad sizes (embedding_size %d, %lld users, %lld entities, %lld candidates, topn %d, nsplit %d)", name, d, (long long)nq,
               (long long)n_ent, (long long)n_cand, topn, nsplit);
  KTUP_REQUIRE(ldu >= d && ldr >= d && lde >= d, "%s: a row pitch is below embedding_size %d", name, d);
  KTUP_REQUIRE(rel >= 0, "%s: negative relation row (got %lld)", name, (long long)rel);
  KTUP_REQUIRE(cand_ids || n_cand == n_ent, "%s: without cand_ids the candidates are the %lld entity rows (got n_cand %lld)", name,
               (long long)n_ent, (long long)n_cand);
  KTUP_REQUIRE((filt_off == nullptr) == (filt_ids == nullptr), "%s: filt_off and filt_ids go together", name);
  KTUP_REQUIRE((reinterpret_cast<uintptr_t>(ws) & 15) == 0, "%s: the workspace must be 16-byte aligned", name);
  if (topn > TOPN_MAX) return set_error(KTUP_ERR_UNSUPPORTED, "%s: topn %d > %d", name, topn, TOPN_MAX);
  if (d > 256) return set_error(KTUP_ERR_UNSUPPORTED, "%s: embedding_size %d > 256", name, d);
  if (n_cand >= ((int64_t)1 << 31)) return set_error(KTUP_ERR_UNSUPPORTED, "%s: %lld candidates do not fit 32-bit ids", name, (long long)n_cand);
  if (nq == 0) return KTUP_OK;
  hipStream_t st = (hipStream_t)stream;
  CfkgPassArgs a;
  a.U = U; a.ldu = ldu; a.R = R; a.ldr = ldr; a.rel = rel; a.E = E; a.lde = lde; a.n_ent = n_ent; a.cand_ids = cand_ids; a.d = d;
  a.evec = (d % 4 == 0 && lde % 4 == 0 && (reinterpret_cast<uintptr_t>(E) & 15) == 0) ? 1 : 0;
  a.u_ids = u_ids; a.nq = nq; a.n_cand = n_cand;
  a.topn = topn;
  a.nsplit = cfkg_nsplit(nq, n_cand, nsplit, &a.split_items);
  a.part = reinterpret_cast<uint64_t*>(ws);
  a.bm = nullptr;
  a.bm_words = (n_cand + 31) / 32;
  a.enorm = nullptr;
  const int64_t nub = (nq + 63) / 64;
  if (nub * a.nsplit > 0x7fffffffLL) return set_error(KTUP_ERR_UNSUPPORTED, "%s: too many users for one call (%lld)", name, (long long)nq);
  // workspace: the partial lists (8-byte entries) | the filter bits | |e|^2 per candidate
  uint32_t* bm = reinterpret_cast<uint32_t*>(a.part + (size_t)nq * a.nsplit * topn);
  const int64_t nw = nq * a.bm_words;
  if (filt_off) {
    hipLaunchKernelGGL(cfkg_filter_zero_kernel, dim3((unsigned)min((nw + 255) / 256, (int64_t)4096)), dim3(256), 0, st, bm, nw);
    if (int rc = check_launch(name)) return rc;
    hipLaunchKernelGGL(cfkg_filter_bits_kernel, dim3((unsigned)min((nq + 3) / 4, (int64_t)4096)), dim3(256), 0, st, filt_off, filt_ids, nq, n_cand,
                       bm, a.bm_words);
    if (int rc = check_launch(name)) return rc;
    a.bm = bm;
  }
  if (!l1) {
    float* en = reinterpret_cast<float*>(bm + nw);
    hipLaunchKernelGGL(cfkg_cand_norm_kernel, dim3((unsigned)min((n_cand + 15) / 16, (int64_t)4096)), dim3(256), 0, st, E, lde, n_ent, cand_ids,
                       n_cand, d, en);
    if (int rc = check_launch(name)) return rc;
    a.enorm = en;
  }
  const unsigned blocks = (unsigned)(nub * a.nsplit);
  const int nk = (d + 3) / 4;
  const bool is_l1 = l1 != 0;
  int rc;
  if (nk <= 5) rc = launch_cfkg_pass<5>(a, is_l1, blocks, st, name);
  else if (nk <= 9) rc = launch_cfkg_pass<9>(a, is_l1, blocks, st, name);
  else if (nk <= 16) rc = launch_cfkg_pass<16>(a, is_l1, blocks, st, name);
  else if (nk <= 25) rc = launch_cfkg_pass<25>(a, is_l1, blocks, st, name);
  else if (nk <= 32) rc = launch_cfkg_pass<32>(a, is_l1, blocks, st, name);
  else if (nk <= 48) rc = launch_cfkg_pass<48>(a, is_l1, blocks, st, name);
  else rc = launch_cfkg_pass<64>(a, is_l1, blocks, st, name);
  if (rc) return rc;
  hipLaunchKernelGGL((topk_merge_kernel<MERGE_PER_LANE, false>), dim3((unsigned)((nq + 3) / 4)), dim3(MERGE_T), 0, st, a.part, nq, a.nsplit, topn, top_ids,
                     top_scores);
  return check_launch(name);
}
