// TransD link prediction: all-entity scores (transD.py:78-134) and the whole filtered-rank pass.
//
// Per key i (query entity q, relation r):  a = Ep[q], b = Rp[r], q_perp = E[q] + (E[q] . a) b,
//     c = q_perp - R[r]  (evaluateHead)   or   q_perp + R[r]  (evaluateTail)
// and every candidate e_j is projected with the QUERY's vector a (transD.py:94-98), so
//     score(i, j) = dist( c - e_j - (e_j . a) b ).
// (evaluateTail of the reference names an undefined t_proj_expand, transD.py:127, and raises NameError; the h_proj_expand it
// computes two lines above -- the query's own projection row -- is the evident intent and what runs here.)
//
// transd_query_prep_kernel writes per key  QW[i] = [c | a | b]  (3 x round4(d) floats, zero tail) and QS[i] = {|c|^2, b.c, |b|^2, 0}.
// Two routes behind ktup_eval_transd_scores:
//   * pair route (L1, any width; squared L2 where the matrix-core route does not apply): 64 candidates staged transposed in
//     LDS (lane <-> candidate, conflict-free b128 reads), the four waves of a workgroup take different keys, QB = 4 at a time,
//     whose vectors arrive through scalar loads.  Pass 1: s = e . a, pass 2: sum dist(c - e - s b) -- the direct form.
//   * matrix-core route (squared L2, d in {20, 36, 64, 100, 128}): the score expands into three (keys x candidates) products,
//         |c - e - (e.a) b|^2 = |c|^2 - 2 [c.e] + |e|^2 - 2 [a.e] (b.c - [b.e]) + [a.e]^2 |b|^2,
//     all three formed per 64 x 64 tile on v_mfma_f32_16x16x4_f32 with fp32 accumulation.  [b.e] depends on (relation, candidate)
//     only; it is still a third product per tile rather than a relation x candidate table built once per call: the kernel is
//     bound by writing the score matrix, not by the matrix cores, the b rows ride in the stage the c and a rows need anyway, and a
//     table would cost a launch, n_rel x n_cand floats of workspace, a relation-id gather in the epilogue and would tie the
//     candidate slice of a sharded pass to a per-slice table.
// The whole pass comes in two forms with the same integers: ktup_eval_kg_ranks_transd (the score matrix of a chunk of keys at a time +
// ktup_eval_gold_ranks) and ktup_eval_kg_ranks_transd_fused (no score matrix: counts formed by the same device code where the scores
// are made, see "the pass without the score matrix" below).
#include <hip/hip_runtime.h>

#include <cstdint>
#include <type_traits>

#include "ktup_common.h"
#include "ktup_lane_swap.h"
#include "ktup_pref_geom.h"
#include "ktup_topn.h"

using namespace ktup;

namespace {

constexpr int CT = 64;   // candidates per workgroup tile
constexpr int QB = 4;    // keys a wave scores together (each LDS read serves QB keys)
constexpr int NWV = 4;   // waves per workgroup of the pair kernel

inline int round4(int d) { return (d + 3) / 4 * 4; }
inline size_t qw_floats(int d, int64_t nq) { return (size_t)nq * 3 * round4(d); }

// One wave per key.
__global__ __launch_bounds__(256) void transd_query_prep_kernel(const float* __restrict__ E, int64_t lde, const float* __restrict__ Ep,
                                                                int64_t ldep, const float* __restrict__ R, int64_t ldr,
                                                                const float* __restrict__ Rp, int64_t ldrp, int d, int dq,
                                                                const int64_t* __restrict__ q, const int64_t* __restrict__ r, int64_t nq,
                                                                int head, float* __restrict__ QW, float* __restrict__ QS) {
  const int lane = threadIdx.x & 63;
  const float sgn = head ? -1.f : 1.f;
  for (int64_t i = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); i < nq; i += (int64_t)gridDim.x * 4) {
    const float* e = E + q[i] * lde;
    const float* a = Ep + q[i] * ldep;
    const float* rel = R + r[i] * ldr;
    const float* b = Rp + r[i] * ldrp;
    float* out = QW + i * 3 * dq;
    float dot = 0.f;
    for (int k = lane; k < d; k += 64) dot = fmaf(e[k], a[k], dot);
    dot = group_sum<64>(dot);
    float cc = 0.f, bc = 0.f, bb = 0.f;
    for (int k = lane; k < dq; k += 64) {
      float c = 0.f, av = 0.f, bv = 0.f;
      if (k < d) { av = a[k]; bv = b[k]; c = fmaf(dot, bv, e[k]) + sgn * rel[k]; }
      out[k] = c; out[dq + k] = av; out[2 * dq + k] = bv;
      cc = fmaf(c, c, cc); bc = fmaf(bv, c, bc); bb = fmaf(bv, bv, bb);
    }
    cc = group_sum<64>(cc); bc = group_sum<64>(bc); bb = group_sum<64>(bb);
    if (lane == 0) { QS[i * 4 + 0] = cc; QS[i * 4 + 1] = bc; QS[i * 4 + 2] = bb; QS[i * 4 + 3] = 0.f; }
  }
}

// ------------------------------------------------------------------------------------------------------------ pair route
struct PairArgs {
  const float* C; int64_t ldc; int64_t n_cand;
  const float* QW; int64_t nq;
  int d, dq; bool cvec;
  float* out; int64_t ldo;
  // COUNT / list forms: the pass's CSR lists, the list scores and the per-gold counts
  int descending;
  const int64_t* gold_off; const int32_t* gold_ids; float* gscore;
  const int64_t* filt_off; const int32_t* filt_ids; float* fscore;
  int32_t* counts;
};

typedef float v2f __attribute__((ext_vector_type(2)));
KTUP_DEV v2f lo2(float4 a) { return v2f{a.x, a.y}; }
KTUP_DEV v2f hi2(float4 a) { return v2f{a.z, a.w}; }
KTUP_DEV v2f fma2(v2f a, v2f b, v2f c) { return __builtin_elementwise_fma(a, b, c); }

KTUP_DEV float4 load_cand4(const float* base, int64_t ld, int64_t row, int c, int d, bool vec) {
  const float* p = base + row * ld + 4 * c;
  if (vec) return *reinterpret_cast<const float4*>(p);
  float4 v;
  v.x = 4 * c + 0 < d ? p[0] : 0.f;
  v.y = 4 * c + 1 < d ? p[1] : 0.f;
  v.z = 4 * c + 2 < d ? p[2] : 0.f;
  v.w = 4 * c + 3 < d ? p[3] : 0.f;
  return v;
}

// where a candidate's float4 chunk c comes from: the workgroup's LDS stage (lane <-> candidate) or the row itself (list form)
struct StagedCand {
  const float4* cand; int lane;
  KTUP_DEV float4 operator()(uint32_t c) const { return cand[c * CT + lane]; }
};
struct RowCand {
  const float* row; int d; bool vec;
  KTUP_DEV float4 operator()(uint32_t c) const { return load_cand4(row, 0, 0, (int)c, d, vec); }
};

// The per-pair arithmetic of the pair route, for NQ keys (vectors through scalar loads) against this lane's candidate: pass 1
// s = -(e . a), pass 2 sum dist((c - e) + s b).  ONE copy for the score kernel, its COUNT form and the list kernel: the same
// instructions on the same operands, so a (key, candidate) pair has the same bits wherever it is scored.
template <bool L1, int NQ, class Cand>
KTUP_DEV void transd_pair_scores(const Cand& cand, int nch4, const sptr4* qc, const sptr4* qa, const sptr4* qb, float* out) {
  v2f s2[NQ], a2[NQ];
  float acc[NQ];
#pragma unroll
  for (int qi = 0; qi < NQ; ++qi) { s2[qi] = v2f{0.f, 0.f}; a2[qi] = v2f{0.f, 0.f}; acc[qi] = 0.f; }
#pragma unroll 2
  for (uint32_t c = 0; c < (uint32_t)nch4; ++c) {          // pass 1: -(e . a)
    const float4 e = cand(c);
#pragma unroll
    for (int qi = 0; qi < NQ; ++qi) {
      const float4 av = sldp(qa[qi] + c);
      s2[qi] = fma2(-lo2(e), lo2(av), s2[qi]);
      s2[qi] = fma2(-hi2(e), hi2(av), s2[qi]);
    }
  }
  v2f ms[NQ];
#pragma unroll
  for (int qi = 0; qi < NQ; ++qi) { const float s = s2[qi].x + s2[qi].y; ms[qi] = v2f{s, s}; }
#pragma unroll 2
  for (uint32_t c = 0; c < (uint32_t)nch4; ++c) {          // pass 2: z = (c - e) - (e . a) b
    const float4 e = cand(c);
#pragma unroll
    for (int qi = 0; qi < NQ; ++qi) {
      const float4 cv = sldp(qc[qi] + c), bv = sldp(qb[qi] + c);
      const v2f zl = fma2(ms[qi], lo2(bv), lo2(cv) - lo2(e)), zh = fma2(ms[qi], hi2(bv), hi2(cv) - hi2(e));
      if constexpr (L1) {
        acc[qi] += (fabsf(zl.x) + fabsf(zl.y)) + (fabsf(zh.x) + fabsf(zh.y));
      } else {
        a2[qi] = fma2(zl, zl, a2[qi]);
        a2[qi] = fma2(zh, zh, a2[qi]);
      }
    }
  }
#pragma unroll
  for (int qi = 0; qi < NQ; ++qi) out[qi] = L1 ? acc[qi] : a2[qi].x + a2[qi].y;
}

// COUNT = false: scores to a.out.  COUNT = true (the pass without the score matrix): per gold entry of a key the number of this
// tile's candidates whose 64-bit key is below the gold's -- a wave reduction per (key, gold); the counts of a key group's first TH
// golds per key collect in one register (lane qi * TH + k) and leave as ONE atomic instruction.
constexpr int TH = 4;
template <bool L1, bool COUNT>
__global__ __launch_bounds__(NWV * 64) void transd_pairs_kernel(PairArgs a) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  float4* cand = reinterpret_cast<float4*>(smem);          // [nch4][CT]
  const int t = threadIdx.x, lane = t & 63;
  const int w = __builtin_amdgcn_readfirstlane(t >> 6);
  const int nch4 = a.dq / 4;
  const int64_t j0 = (int64_t)blockIdx.x * CT;
  for (int idx = t; idx < nch4 * CT; idx += NWV * 64) {
    const int j = idx & (CT - 1), c = idx >> 6;
    const int64_t gj = min(j0 + j, a.n_cand - 1);            // (rows past the end repeat the last one; never stored or counted)
    cand[c * CT + j] = load_cand4(a.C, a.ldc, gj, c, a.d, a.cvec);
  }
  __syncthreads();
  const sptr4 QW = as_scalar(a.QW);
  // this workgroup's slice of the keys (grid.y splits them), QB at a time per wave
  const int64_t per = ((a.nq + gridDim.y - 1) / gridDim.y + NWV * QB - 1) / (NWV * QB) * (NWV * QB);
  const int64_t qlo = (int64_t)blockIdx.y * per, qhi = min(a.nq, qlo + per);
  for (int64_t b0 = qlo + w * QB; b0 < qhi; b0 += NWV * QB) {
    sptr4 qc[QB], qa[QB], qb[QB];
#pragma unroll
    for (int qi = 0; qi < QB; ++qi) {
      const int64_t pos = min(b0 + qi, a.nq - 1);
      qc[qi] = QW + pos * 3 * nch4;
      qa[qi] = qc[qi] + nch4;
      qb[qi] = qc[qi] + 2 * nch4;
    }
    float sc[QB];
    transd_pair_scores<L1, QB>(StagedCand{cand, lane}, nch4, qc, qa, qb, sc);
    if constexpr (COUNT) {
      static_assert(QB * TH <= 64, "lane qi * TH + k <-> (key of the group, gold slot)");
      const bool desc = a.descending != 0;
      const bool in = j0 + lane < a.n_cand;
      int cntv = 0;
      int64_t slot = 0;
#pragma unroll
      for (int qi = 0; qi < QB; ++qi) {
        if (b0 + qi >= qhi) break;                           // (uniform)
        const int64_t g0 = a.gold_off[b0 + qi], g1 = a.gold_off[b0 + qi + 1];
        if ((lane >> 2) == qi) slot = g0 + (lane & 3);
        const uint64_t ck = topn_key(sc[qi], desc, (uint32_t)(j0 + lane));
        for (int64_t g = g0; g < g1; ++g) {                  // a key's golds: uniform, through scalar loads
          const int32_t gid = a.gold_ids[g];
          if (gid < 0 || gid >= a.n_cand) continue;
          const uint64_t gk = topn_key(a.gscore[g], desc, (uint32_t)gid);
          const int n = (int)__popcll(__builtin_amdgcn_ballot_w64(in && ck < gk));
          if (g - g0 < TH) cntv = lane == qi * TH + (int)(g - g0) ? n : cntv;
          else if (n != 0 && lane == 0) atomicAdd(a.counts + g, n);
        }
      }
      if (lane < QB * TH && cntv != 0) atomicAdd(a.counts + slot, cntv);
    } else {
      if (j0 + lane < a.n_cand) {
#pragma unroll
        for (int qi = 0; qi < QB; ++qi)
          if (b0 + qi < qhi) a.out[(b0 + qi) * a.ldo + j0 + lane] = sc[qi];
      }
    }
  }
}

// The scores of every key's OWN list entries (golds, then filtered ids) with transd_pair_scores: a wave takes one key at a time and
// scores up to 64 of its entries (lane <-> entry), every lane reading its entry's row where it lies -- no LDS stage, for the reason
// ktup_eval.hip's pairs_list_kernel gives (the staged form was a chain of exposed latencies and held a CU to a few waves).
template <bool L1>
__global__ __launch_bounds__(NWV * 64) void transd_pairs_list_kernel(PairArgs a) {
  const int lane = threadIdx.x & 63;
  const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int nch4 = a.dq / 4;
  const sptr4 QW = as_scalar(a.QW);
  for (int64_t key = (int64_t)blockIdx.x * NWV + w; key < a.nq; key += (int64_t)gridDim.x * NWV) {
    const int64_t g0 = a.gold_off[key], ng = a.gold_off[key + 1] - g0;
    const int64_t f0 = a.filt_off ? a.filt_off[key] : 0, nf = a.filt_off ? a.filt_off[key + 1] - f0 : 0;
    const sptr4 qc[1] = {QW + key * 3 * nch4}, qa[1] = {qc[0] + nch4}, qb[1] = {qc[0] + 2 * nch4};
    for (int64_t base = 0; base < ng + nf; base += 64) {
      const int64_t e = base + lane;
      const bool on = e < ng + nf;
      const int32_t cid = !on ? 0 : (e < ng ? a.gold_ids[g0 + e] : a.filt_ids[f0 + (e - ng)]);
      const bool valid = on && cid >= 0 && cid < a.n_cand;
      float sc[1];
      transd_pair_scores<L1, 1>(RowCand{a.C + (int64_t)(valid ? cid : 0) * a.ldc, a.d, a.cvec}, nch4, qc, qa, qb, sc);
      if (valid) {
        if (e < ng) a.gscore[g0 + e] = sc[0]; else a.fscore[f0 + (e - ng)] = sc[0];
      }
    }
  }
}

// grid.y splits the keys: about `target` workgroups for a short call, up to 8 rounds of the chip's slots for a long one, every
// split a whole number of NWV x QB key groups.
dim3 pairs_grid(int64_t n_cand, int64_t nq) {
  const int64_t tiles = (n_cand + CT - 1) / CT, group = NWV * QB, slots = 1536;
  const int64_t ymax = (nq + group - 1) / group;
  int64_t target = 2048;
  const int64_t fine = tiles * ymax / 6;
  if (fine > target) target = fine < 8 * slots ? fine : 8 * slots;
  int64_t ysplit = (target + tiles - 1) / tiles;
  if (ysplit > ymax) ysplit = ymax;
  if (ysplit < 1) ysplit = 1;
  const int64_t per = ((nq + ysplit - 1) / ysplit + group - 1) / group * group;
  ysplit = (nq + per - 1) / per;
  return dim3((unsigned)tiles, (unsigned)(ysplit < 1 ? 1 : ysplit));
}

inline size_t pairs_lds(int dq) { return (size_t)(dq / 4) * CT * 16; }

template <bool L1, bool COUNT>
int launch_pairs_form(const PairArgs& a, hipStream_t st, const char* name) {
  const size_t lds = pairs_lds(a.dq);
  if (lds > 160 * 1024) return set_error(KTUP_ERR_UNSUPPORTED, "%s: embedding_size %d needs %zu B of LDS", name, a.d, lds);
  const dim3 grid = pairs_grid(a.n_cand, a.nq);
  if (grid.y > 65535) return set_error(KTUP_ERR_UNSUPPORTED, "%s: too many keys for one call (%lld)", name, (long long)a.nq);
  if (lds > 64 * 1024) (void)hipFuncSetAttribute((const void*)transd_pairs_kernel<L1, COUNT>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  if constexpr (COUNT)    // the list scores first: the count form compares against them
    hipLaunchKernelGGL((transd_pairs_list_kernel<L1>), dim3(grid_for((a.nq + NWV - 1) / NWV, 8192)), dim3(NWV * 64), 0, st, a);
  hipLaunchKernelGGL((transd_pairs_kernel<L1, COUNT>), grid, dim3(NWV * 64), lds, st, a);
  return check_launch(name);
}

int launch_pairs(const PairArgs& a, int l1, hipStream_t st, const char* name) {
  return l1 ? launch_pairs_form<true, false>(a, st, name) : launch_pairs_form<false, false>(a, st, name);
}
int launch_pairs_count(const PairArgs& a, int l1, hipStream_t st, const char* name) {
  return l1 ? launch_pairs_form<true, true>(a, st, name) : launch_pairs_form<false, true>(a, st, name);
}

// ------------------------------------------------------------------------------------------------------ matrix-core route
constexpr int IB = 64;   // candidates per workgroup

template <int NCH_>
struct DGeom {
  static constexpr int NCH = NCH_, D = 4 * NCH;
  static constexpr int KG = (D + 15) / 16;
  static constexpr bool TAIL1 = NCH - 4 * (KG - 1) == 1;       // d % 16 == 4: the last chunk goes through one b32-operand MFMA
  static constexpr int KGF = TAIL1 ? KG - 1 : KG;
  static_assert(TAIL1 || NCH % 4 == 0, "k groups must be whole (d % 16 in {0, 4})");
  static constexpr int P4 = NCH | 1;                           // odd float4 row pitch: conflict-free b128 operand reads
  static constexpr int QV = 3;                                 // vectors per key: c, a, b
  static constexpr int UB = 64, NW = 16;
  static constexpr size_t LDS = (size_t)(UB * QV + IB) * P4 * 16 + (size_t)IB * 4;
  static_assert(LDS <= 160 * 1024, "LDS budget");
};

struct McArgs {
  const float* QW; const float* QS;
  const float* C; int64_t ldc;
  int64_t nq, n_cand;
  float* out; int64_t ldo;
};

// ---- pieces shared by the score kernel, the list kernel and the count sweep: identical code => identical bits
// |e|^2 of a candidate row: 8 lanes per row take chunks sub, sub + 8, ...; all eight get the sum
KTUP_DEV float row_norm8(const v4* r0, int nch, int sub) {
  v4 s0 = (v4){0.f, 0.f, 0.f, 0.f};
  for (int c = sub; c < nch; c += 8) { const v4 x0 = r0[c]; s0 += x0 * x0; }
  float f0 = (s0[0] + s0[1]) + (s0[2] + s0[3]);
#pragma unroll
  for (int m = 1; m < 8; m <<= 1) f0 += __shfl_xor(f0, m, 64);
  return f0;
}

// one 16 x 16 (keys x candidates) tile of the three products: qrow = the lane's key row [QV][P4] (c | a | b), crow = its candidate
// row; lane (kq, j) feeds k-slot kq
template <typename G>
KTUP_DEV void tile_dots3(const v4* qrow, const v4* crow, int kq, v4& ce, v4& ae, v4& be) {
  constexpr int KGF = G::KGF, P4 = G::P4;
  const v4* qa = qrow + kq;                                    // c at +0, a at +P4, b at +2 P4
  const v4* cb = crow + kq;
  ce = (v4){0.f, 0.f, 0.f, 0.f}; ae = ce; be = ce;
#pragma unroll
  for (int g = 0; g < KGF; ++g) {
    const v4 xc = qa[4 * g], xa = qa[P4 + 4 * g], xb = qa[2 * P4 + 4 * g], xe = cb[4 * g];
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      ce = __builtin_amdgcn_mfma_f32_16x16x4f32(xc[c], xe[c], ce, 0, 0, 0);
      ae = __builtin_amdgcn_mfma_f32_16x16x4f32(xa[c], xe[c], ae, 0, 0, 0);
      be = __builtin_amdgcn_mfma_f32_16x16x4f32(xb[c], xe[c], be, 0, 0, 0);
    }
  }
  if (G::TAIL1) {                                              // coordinates 16 KGF + kq
    const float* qf = reinterpret_cast<const float*>(qrow + 4 * KGF) + kq;
    const float xe = (reinterpret_cast<const float*>(crow + 4 * KGF) + kq)[0];
    ce = __builtin_amdgcn_mfma_f32_16x16x4f32(qf[0], xe, ce, 0, 0, 0);
    ae = __builtin_amdgcn_mfma_f32_16x16x4f32(qf[4 * P4], xe, ae, 0, 0, 0);
    be = __builtin_amdgcn_mfma_f32_16x16x4f32(qf[8 * P4], xe, be, 0, 0, 0);
  }
}

// the expansion of the file header from the three products, qs = {|c|^2, b.c, |b|^2}, ee = |e|^2
KTUP_DEV float mc_score(float ce, float ae, float be, v4 qs, float ee) {
  const float s = ae;
  float score = fmaf(-2.f, ce, qs[0] + ee);
  score = fmaf(s, fmaf(s, qs[2], -2.f * (qs[1] - be)), score);
  return score;
}

template <typename G>
__global__ __launch_bounds__(G::NW * 64) void transd_l2_mc_kernel(McArgs a) {
  constexpr int NCH = G::NCH, UB = G::UB, P4 = G::P4, NW = G::NW, QV = G::QV, D = G::D;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  v4* Q = reinterpret_cast<v4*>(smem);                         // [UB][QV][P4]
  v4* Cd = Q + UB * QV * P4;                                   // [IB][P4]
  float* cs = reinterpret_cast<float*>(Cd + IB * P4);          // [IB]: |e|^2
  const int tid = threadIdx.x, lane = tid & 63, kq = lane >> 4, j = lane & 15;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  // XCD-aware tile order: consecutive workgroups go round-robin to the 8 XCDs; each XCD gets a contiguous band of candidate
  // tiles, so its L2 holds its band and the (small) key block.  grid.x is padded to 8 bands of nxp tiles.
  const int nxp = gridDim.x >> 3;
  const int bid = blockIdx.y * gridDim.x + blockIdx.x, xcd = bid & 7, local = bid >> 3;
  const int tx = xcd * nxp + local % nxp, ty = local / nxp;
  if ((int64_t)tx * IB >= a.n_cand) return;
  const int64_t u0 = (int64_t)ty * UB, i0 = (int64_t)tx * IB;
  for (int idx = tid; idx < UB * QV * NCH; idx += NW * 64) {
    const int row = idx / (QV * NCH), rem = idx - row * (QV * NCH), vec = rem / NCH, c = rem - vec * NCH;
    v4 val = (v4){0.f, 0.f, 0.f, 0.f};
    if (u0 + row < a.nq) val = *reinterpret_cast<const v4*>(a.QW + ((u0 + row) * 3 + vec) * D + 4 * c);
    Q[(row * QV + vec) * P4 + c] = val;
  }
  for (int idx = tid; idx < IB * NCH; idx += NW * 64) {
    const int row = idx / NCH, c = idx - row * NCH;
    v4 val = (v4){0.f, 0.f, 0.f, 0.f};
    if (i0 + row < a.n_cand) val = *reinterpret_cast<const v4*>(a.C + (i0 + row) * a.ldc + 4 * c);
    Cd[row * P4 + c] = val;
  }
  __syncthreads();
  for (int row = tid >> 3; row < IB; row += (NW * 64) >> 3) {  // |e|^2, 8 lanes per candidate
    const float f0 = row_norm8(Cd + row * P4, NCH, tid & 7);
    if ((tid & 7) == 0) cs[row] = f0;
  }
  __syncthreads();
  // this wave's 16 x 16 tile: keys are MFMA rows (A operand), candidates columns (B operand)
  const int ut = w >> 2, it = w & 3;
  v4 ce, ae, be;
  tile_dots3<G>(Q + ((16 * ut + j) * QV) * P4, Cd + (16 * it + j) * P4, kq, ce, ae, be);
  // epilogue: lane (kq, j) holds keys 16 ut + 4 kq + reg (reg = 0..3) x candidate 16 it + j
  const float ee = cs[16 * it + j];
  const int64_t cnd = i0 + 16 * it + j;
#pragma unroll
  for (int reg = 0; reg < 4; ++reg) {
    const int64_t key = u0 + 16 * ut + 4 * kq + reg;
    if (key < a.nq && cnd < a.n_cand) {
      const v4 qs = *reinterpret_cast<const v4*>(a.QS + key * 4);       // |c|^2, b.c, |b|^2
      a.out[key * a.ldo + cnd] = mc_score(ce[reg], ae[reg], be[reg], qs, ee);
    }
  }
}

template <typename G>
int launch_mc(const McArgs& a, hipStream_t st, const char* name) {
  (void)hipFuncSetAttribute((const void*)transd_l2_mc_kernel<G>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)G::LDS);
  const unsigned nx = (unsigned)((a.n_cand + IB - 1) / IB), nxp = (nx + 7) / 8;       // 8 XCD bands of nxp candidate tiles
  const dim3 grid(8 * nxp, (unsigned)((a.nq + G::UB - 1) / G::UB));
  hipLaunchKernelGGL((transd_l2_mc_kernel<G>), grid, dim3(G::NW * 64), G::LDS, st, a);
  return check_launch(name);
}

// KTUP_OK / an error, or 1 when the shape is not one of the instantiated ones (the caller runs the pair kernel).
int transd_l2_mc(const McArgs& a, int d, int dq, hipStream_t st, const char* name) {
  if (!aligned16(a.QW) || !aligned16(a.QS) || !aligned16(a.C) || (a.ldc & 3) || dq != d) return 1;
  if ((a.nq + 63) / 64 > 65535) return 1;
  switch (d) {
    case 20: return launch_mc<DGeom<5>>(a, st, name);
    case 36: return launch_mc<DGeom<9>>(a, st, name);
    case 64: return launch_mc<DGeom<16>>(a, st, name);
    case 100: return launch_mc<DGeom<25>>(a, st, name);
    case 128: return launch_mc<DGeom<32>>(a, st, name);
    default: return 1;
  }
}

size_t score_bytes(int64_t chunk, int64_t n_cand) { return (((size_t)chunk * (size_t)n_cand * sizeof(float)) + 255) & ~(size_t)255; }

// double-buffered pass: the rank kernel of chunk c on the library's side stream beside the score kernel of chunk c + 1
struct Ev {
  hipEvent_t ready[2] = {nullptr, nullptr}, done[2] = {nullptr, nullptr};
  bool tried = false, ok = false;
} g_ev;

bool events_ok() {
  if (!g_ev.tried) {
    g_ev.tried = true;
    g_ev.ok = true;
    for (int i = 0; i < 2; ++i)
      if (hipEventCreateWithFlags(&g_ev.ready[i], hipEventDisableTiming) != hipSuccess ||
          hipEventCreateWithFlags(&g_ev.done[i], hipEventDisableTiming) != hipSuccess) {
        (void)hipGetLastError();
        g_ev.ok = false;
      }
  }
  return g_ev.ok;
}

// ------------------------------------------------------------------------------- the pass without the score matrix (squared L2)
// ktup_eval_kg_fused.hip's scheme for TransD: rank(g) = #{c : key(c) < key(g)} - #{c in filter(q) U gold(q), c != g : key(c) < key(g)}.
// There is no fp64 referee here: the chunked route ranks by the fp32 scores of transd_l2_mc_kernel, and this pass forms the SAME
// scores (tile_dots3, row_norm8, mc_score on the same operands), so its integers are the chunked route's.
//   transd_pass_init_kernel    counts <- 0, |e|^2 of every candidate once per pass (the score kernel's 8-lane reduction)
//   transd_list_scores_kernel  the scores of every (key, gold) and (key, filtered id) pair: 16 keys x 16 gathered rows per MFMA tile,
//                              the diagonal kept
//   transd_count_mc_kernel     the sweep: 64 keys' [c | a | b] rows resident in LDS, one band of the candidate table per XCD, 64
//                              candidates per stage; a wave owns a 16 x 16 tile per stage and compares its four scores per lane with
//                              the (<= GS) gold scores of its keys as floats; a tie or a NaN (the gold itself, once per band) goes
//                              to the 64-bit keys; counts in registers, one flush of int atomics per workgroup
// and the finalize step of ktup_eval_kg_fused.hip (kg_rank_finalize).
constexpr int GS = 4, NBAND = 8;   // golds a sweep launch counts for (further launches take golds 4.., 8.. of the keys that have them)

template <int NCH_>
struct PGeom : DGeom<NCH_> {
  using B = DGeom<NCH_>;
  static constexpr size_t KEYS = (size_t)B::UB * GS * 4 + (size_t)B::UB * GS * 8;          // gth [UB][GS] | gkey [UB][GS] u64
  static constexpr size_t STAGE = (size_t)IB * B::P4 * 16, QROWS = (size_t)B::UB * B::QV * B::P4 * 16;
  // three vectors per key: 64 keys and a double-buffered stage are (192 + 128) x 33 x 16 B = 168,960 B at d = 128, over the 160 KB
  // of LDS; that width keeps ONE stage buffer (a second barrier per stage), (192 + 64) x 33 x 16 B = 135,168 B.  d = 100: 128,000 B.
  static constexpr int NBUF = QROWS + 2 * STAGE + KEYS <= 160 * 1024 ? 2 : 1;
  static constexpr size_t LDS = QROWS + NBUF * STAGE + KEYS;
  static_assert(LDS <= 160 * 1024, "LDS budget of the sweep");
  static_assert(NCH_ != 32 || (NBUF == 1 && LDS == 135168 + 3072), "d = 128: single-buffered stage");
  static_assert(NCH_ != 25 || (NBUF == 2 && LDS == 128000 + 3072), "d = 100: double-buffered stage");
  static constexpr size_t LIST_LDS = QROWS + STAGE;                                        // list kernel: Q | [4 waves][16][P4]
};

struct PassArgs {
  const float* QW; const float* QS;
  const float* C; int64_t ldc;
  int64_t nq, n_cand;
  int descending;
  const int64_t* gold_off; const int32_t* gold_ids; float* gscore;
  const int64_t* filt_off; const int32_t* filt_ids; float* fscore;
  int32_t* counts;
  const float* cnorm;
  int tiles_per_band, gbase;
};

__global__ __launch_bounds__(256) void transd_pass_init_kernel(int32_t* counts, int64_t n, const float* __restrict__ C, int64_t ldc, int nch,
                                                               int64_t n_cand, float* __restrict__ cnorm) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) counts[i] = 0;
  for (int64_t row = ((int64_t)blockIdx.x * 256 + threadIdx.x) >> 3; row < n_cand; row += ((int64_t)gridDim.x * 256) >> 3) {
    const float f0 = row_norm8(reinterpret_cast<const v4*>(C + row * ldc), nch, threadIdx.x & 7);
    if ((threadIdx.x & 7) == 0) cnorm[row] = f0;
  }
}

template <typename G>
KTUP_DEV void stage_keys(const PassArgs& a, v4* Q, int64_t u0, int nthreads) {
  constexpr int NCH = G::NCH, QV = G::QV, P4 = G::P4, D = G::D;
  for (int idx = threadIdx.x; idx < G::UB * QV * NCH; idx += nthreads) {
    const int row = idx / (QV * NCH), rem = idx - row * (QV * NCH), vec = rem / NCH, c = rem - vec * NCH;
    v4 val = (v4){0.f, 0.f, 0.f, 0.f};
    if (u0 + row < a.nq) val = *reinterpret_cast<const v4*>(a.QW + ((u0 + row) * 3 + vec) * D + 4 * c);
    Q[(row * QV + vec) * P4 + c] = val;
  }
}

// one wave per 16 keys; round s scores every key of the wave against the s-th entry of ITS OWN list (golds first, then filtered
// ids).  4 waves = 64 keys per workgroup share the key stage.  Ids are fetched two rounds ahead and rows one round ahead.
template <typename G>
__global__ __launch_bounds__(256) void transd_list_scores_kernel(PassArgs a) {
  constexpr int NCH = G::NCH, P4 = G::P4, QV = G::QV, UB = G::UB;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  v4* Q = reinterpret_cast<v4*>(smem);                         // [UB][QV][P4]
  v4* Cd = Q + UB * QV * P4;                                   // [4 waves][16][P4]
  const int tid = threadIdx.x, lane = tid & 63, kq = lane >> 4, j = lane & 15;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int64_t u0 = (int64_t)blockIdx.x * UB;
  stage_keys<G>(a, Q, u0, 256);
  __syncthreads();
  const int64_t key_j = u0 + 16 * w + j;                        // this lane's key for gathering: lane = (row j of the wave, chunk group)
  const bool key_on = key_j < a.nq;
  const int64_t g0 = key_on ? a.gold_off[key_j] : 0, ng = key_on ? a.gold_off[key_j + 1] - g0 : 0;
  const int64_t f0_ = (key_on && a.filt_off) ? a.filt_off[key_j] : 0, nf = (key_on && a.filt_off) ? a.filt_off[key_j + 1] - f0_ : 0;
  const v4 qs = key_on ? *reinterpret_cast<const v4*>(a.QS + key_j * 4) : (v4){0.f, 0.f, 0.f, 0.f};
  const int64_t len = ng + nf;
  int64_t maxlen = len;
#pragma unroll
  for (int m = 1; m < 64; m <<= 1) { const int64_t o = __shfl_xor(maxlen, m, 64); maxlen = o > maxlen ? o : maxlen; }
  v4* myC = Cd + w * 16 * P4;
  constexpr int RN = (NCH + 3) / 4;
  auto list_id = [&](int64_t s) -> int32_t {
    if (s >= len) return -1;
    return s < ng ? a.gold_ids[g0 + s] : a.filt_ids[f0_ + (s - ng)];
  };
  v4 rw[RN];
  float en_n = 0.f;
  auto list_rows = [&](int32_t cid) {
    const bool valid = cid >= 0 && cid < a.n_cand;
#pragma unroll
    for (int k = 0; k < RN; ++k) {
      const int c = kq + 4 * k;
      rw[k] = (valid && c < NCH) ? *reinterpret_cast<const v4*>(a.C + (int64_t)cid * a.ldc + 4 * c) : (v4){0.f, 0.f, 0.f, 0.f};
    }
    en_n = valid ? a.cnorm[cid] : 0.f;                           // the same |e|^2 the sweep reads
  };
  int32_t cid_cur = list_id(0), cid_nxt = list_id(1);
  list_rows(cid_cur);
  for (int64_t s = 0; s < maxlen; ++s) {
    const bool valid = cid_cur >= 0 && cid_cur < a.n_cand;
#pragma unroll
    for (int k = 0; k < RN; ++k)
      if (kq + 4 * k < NCH) myC[j * P4 + kq + 4 * k] = rw[k];
    const float en = en_n;
    const int32_t cid_nn = list_id(s + 2);
    list_rows(cid_nxt);                                          // in flight under this round's MFMAs
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    v4 ce, ae, be;
    tile_dots3<G>(Q + ((16 * w + j) * QV) * P4, myC + j * P4, kq, ce, ae, be);
    // diagonal: key (4 kq + reg) against candidate column j  <=>  j == 4 kq + reg
    const int reg = j - 4 * kq;
    if (reg >= 0 && reg < 4 && valid) {
      float c1 = ce[0], a1 = ae[0], b1 = be[0];
      if (reg == 1) { c1 = ce[1]; a1 = ae[1]; b1 = be[1]; }
      if (reg == 2) { c1 = ce[2]; a1 = ae[2]; b1 = be[2]; }
      if (reg == 3) { c1 = ce[3]; a1 = ae[3]; b1 = be[3]; }
      const float sc = mc_score(c1, a1, b1, qs, en);
      if (s < ng) a.gscore[g0 + s] = sc; else a.fscore[f0_ + (s - ng)] = sc;
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    cid_cur = cid_nxt; cid_nxt = cid_nn;
  }
}

template <typename G>
__global__ __launch_bounds__(G::NW * 64) void transd_count_mc_kernel(PassArgs a) {
  constexpr int NCH = G::NCH, P4 = G::P4, QV = G::QV, UB = G::UB, NW = G::NW, NBUF = G::NBUF;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  v4* Q = reinterpret_cast<v4*>(smem);                          // [UB][QV][P4]
  v4* Cd = Q + UB * QV * P4;                                    // [NBUF][IB][P4]
  float* gth = reinterpret_cast<float*>(Cd + NBUF * IB * P4);   // [UB][GS] gold scores as compared (sign-flipped when descending)
  uint64_t* gkey = reinterpret_cast<uint64_t*>(gth + UB * GS);  // [UB][GS]  (8-byte aligned: every part before is a multiple of 16)
  const int tid = threadIdx.x, lane = tid & 63, kq = lane >> 4, j = lane & 15;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int band = blockIdx.x;                                  // consecutive workgroup ids go round the 8 XCDs: band == XCD
  const int64_t u0 = (int64_t)blockIdx.y * UB;
  const bool desc = a.descending != 0;
  const uint32_t flip = desc ? 0x80000000u : 0u;                // scores are compared as s ^ flip: ascending in every case
  int most = 0;
  if (tid < UB && u0 + tid < a.nq) most = (int)min((int64_t)GS, a.gold_off[u0 + tid + 1] - a.gold_off[u0 + tid] - a.gbase);
  if (!__syncthreads_or(most > 0)) return;                      // no key of this block has a gold in this launch's window
  const bool wg_one = !__syncthreads_or(most > 1), wg_two = !__syncthreads_or(most > 2);
  stage_keys<G>(a, Q, u0, NW * 64);
  for (int idx = tid; idx < UB * GS; idx += NW * 64) {           // gold keys of the 64 keys (0 = no gold: no key is below it)
    const int row = idx / GS, g = a.gbase + idx - row * GS;
    uint64_t k = 0;
    float th = -__builtin_inff();                               // nothing is below it; a tie with it goes to the key compare (skipped)
    if (u0 + row < a.nq) {
      const int64_t g0 = a.gold_off[u0 + row], n = a.gold_off[u0 + row + 1] - g0;
      if (g < n) {
        k = topn_key(a.gscore[g0 + g], desc, (uint32_t)a.gold_ids[g0 + g]);
        th = __uint_as_float(__float_as_uint(a.gscore[g0 + g]) ^ flip);
      }
    }
    gkey[idx] = k; gth[idx] = th;
  }
  __syncthreads();
  const int ut = w >> 2, it = w & 3;
  const v4* qrow = Q + ((16 * ut + j) * QV) * P4;
  auto run = [&](auto gn_c) {
    constexpr int GN = decltype(gn_c)::value;
    int cnt[4][GN];
    float th[4][GN];
    v4 qsr[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int ur = 16 * ut + 4 * kq + r;
#pragma unroll
      for (int g = 0; g < GN; ++g) { cnt[r][g] = 0; th[r][g] = gth[ur * GS + g]; }
      qsr[r] = u0 + ur < a.nq ? *reinterpret_cast<const v4*>(a.QS + (u0 + ur) * 4) : (v4){0.f, 0.f, 0.f, 0.f};
    }
    const int t0 = band * a.tiles_per_band, t1 = t0 + a.tiles_per_band;
    // a thread's share of a 64-candidate stage and its candidate's |e|^2, fetched one stage AHEAD into registers through BUFFER loads:
    // a per-thread byte offset fixed for the whole sweep + the stage's offset, bounds checked by the descriptor (rows past the band's
    // end and stages past the sweep's read as zeros)
    constexpr int NLD = (IB * NCH + NW * 64 - 1) / (NW * 64);
    v4 nx[NLD];
    float en_nx = 0.f;
    const int64_t band_row0 = (int64_t)t0 * IB;
    const int64_t band_rows = max((int64_t)0, min((int64_t)a.tiles_per_band * IB, a.n_cand - band_row0));
    const __amdgpu_buffer_rsrc_t rsC = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(a.C + band_row0 * a.ldc), 0,
                                                                           (int)(band_rows * a.ldc * 4), 0x00020000);
    const __amdgpu_buffer_rsrc_t rsN = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(a.cnorm + band_row0), 0, (int)(band_rows * 4),
                                                                           0x00020000);
    int voC[NLD];
#pragma unroll
    for (int k = 0; k < NLD; ++k) {
      const int idx = tid + k * NW * 64;
      const int row = idx / NCH, c = idx - row * NCH;
      voC[k] = idx < IB * NCH ? (int)((row * a.ldc + 4 * c) * 4) : -16;             // (as unsigned: out of range for every stage -> zeros)
    }
    const int voN = (16 * it + j) * 4;
    const int stepC = (int)(IB * a.ldc * 4);
    auto fetch = [&](int s) {                                     // s = stage index inside the band (uniform)
      const int soC = s * stepC, soN = s * IB * 4;
#pragma unroll
      for (int k = 0; k < NLD; ++k)
        nx[k] = __builtin_bit_cast(v4, __builtin_amdgcn_raw_buffer_load_b128(rsC, voC[k] < 0 ? voC[k] : voC[k] + soC, 0, 0));
      en_nx = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rsN, voN + soN, 0, 0));
    };
    fetch(0);
    for (int t = t0; t < t1; ++t) {
      const int64_t i0 = (int64_t)t * IB;
      if (i0 >= a.n_cand) break;
      // two buffers: the other half was read in stage t - 1 and every wave is past that barrier; one buffer: wait for its readers
      v4* Cs = Cd + (NBUF == 2 ? ((t - t0) & 1) * IB * P4 : 0);
      if (NBUF == 1 && t > t0) __syncthreads();
#pragma unroll
      for (int k = 0; k < NLD; ++k) {
        const int idx = tid + k * NW * 64;
        if (idx < IB * NCH) Cs[(idx / NCH) * P4 + (idx % NCH)] = nx[k];
      }
      const float ee = en_nx;
      fetch(t + 1 - t0);
      __syncthreads();
      v4 ce, ae, be;
      tile_dots3<G>(qrow, Cs + (16 * it + j) * P4, kq, ce, ae, be);
      const int64_t cand = i0 + 16 * it + j;
      if (cand < a.n_cand) {
        float s[4];
        bool tie = false;
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) {
          s[reg] = __uint_as_float(__float_as_uint(mc_score(ce[reg], ae[reg], be[reg], qsr[reg], ee)) ^ flip);
#pragma unroll
          for (int g = 0; g < GN; ++g) {
            const bool lt = s[reg] < th[reg][g];
            cnt[reg][g] += lt ? 1 : 0;
            tie |= !lt && !(s[reg] > th[reg][g]);                 // equal or unordered: the keys decide
          }
        }
        if (__builtin_amdgcn_ballot_w64(tie) != 0) {               // rare: the gold itself (once per band), exact ties, NaNs
#pragma unroll
          for (int reg = 0; reg < 4; ++reg) {
            const int ur = 16 * ut + 4 * kq + reg;
#pragma unroll
            for (int g = 0; g < GN; ++g) {
              if (s[reg] < th[reg][g] || s[reg] > th[reg][g]) continue;
              const uint64_t gk = gkey[ur * GS + g];
              if (gk == 0 || (uint32_t)gk == (uint32_t)cand) continue;          // no such gold; the gold itself is not before itself
              cnt[reg][g] += topn_key(s[reg], false, (uint32_t)cand) < gk ? 1 : 0;      // s is already flipped
            }
          }
        }
      }
    }
    // 16 candidate lanes (j) of a key -> one sum; the lanes with j == 0 flush
#pragma unroll
    for (int reg = 0; reg < 4; ++reg)
#pragma unroll
      for (int g = 0; g < GN; ++g) {
        int c = cnt[reg][g];
#pragma unroll
        for (int m = 1; m < 16; m <<= 1) c += __shfl_xor(c, m, 64);
        cnt[reg][g] = c;
      }
    if (j == 0) {
#pragma unroll
      for (int reg = 0; reg < 4; ++reg) {
        const int64_t key = u0 + 16 * ut + 4 * kq + reg;
        if (key < a.nq) {
          const int64_t g0 = a.gold_off[key], n = a.gold_off[key + 1] - g0;
#pragma unroll
          for (int g = 0; g < GN; ++g)
            if (a.gbase + g < n && cnt[reg][g] != 0) atomicAdd(a.counts + g0 + a.gbase + g, cnt[reg][g]);
        }
      }
    }
  };
  // most keys of a link-prediction pass have one or two golds: such a block runs the loop with one / two compares per score
  if (wg_one) run(std::integral_constant<int, 1>{});
  else if (wg_two) run(std::integral_constant<int, 2>{});
  else run(std::integral_constant<int, GS>{});
}

template <typename G>
int run_pass_mc(PassArgs a, int64_t n_gold, int64_t max_golds, float* cnorm, hipStream_t st, const char* name) {
  const unsigned qblocks = (unsigned)((a.nq + G::UB - 1) / G::UB);
  const int64_t init_work = n_gold > (a.n_cand * 8) ? n_gold : a.n_cand * 8;
  hipLaunchKernelGGL(transd_pass_init_kernel, dim3(grid_for((init_work + 255) / 256, 2048)), dim3(256), 0, st, a.counts, n_gold, a.C, a.ldc,
                     G::NCH, a.n_cand, cnorm);
  (void)hipFuncSetAttribute((const void*)transd_list_scores_kernel<G>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)G::LIST_LDS);
  hipLaunchKernelGGL((transd_list_scores_kernel<G>), dim3(qblocks), dim3(256), G::LIST_LDS, st, a);
  const int64_t ntiles = (a.n_cand + IB - 1) / IB;
  a.tiles_per_band = (int)((ntiles + NBAND - 1) / NBAND);
  (void)hipFuncSetAttribute((const void*)transd_count_mc_kernel<G>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)G::LDS);
  for (a.gbase = 0; a.gbase < max_golds; a.gbase += GS)        // typical keys have one to three golds: one launch; the blocks of a
    hipLaunchKernelGGL((transd_count_mc_kernel<G>), dim3(NBAND, qblocks), dim3(G::NW * 64), G::LDS, st, a);   // later one without such golds exit
  return check_launch(name);
}

// the sweep's shapes: the score kernel's (transd_l2_mc), a candidate band behind one 32-bit buffer descriptor
bool pass_mc_covers(int d, int l1, const float* C, int64_t ldc, int64_t n_cand) {
  return !l1 && ktup::opt_eval_mc() && (d == 20 || d == 36 || d == 64 || d == 100 || d == 128) && aligned16(C) && (ldc & 3) == 0 &&
         ((n_cand + IB * NBAND - 1) / (IB * NBAND) + 1) * IB * ldc * 4 < (1ll << 31);
}

size_t pad256(size_t n) { return (n + 255) & ~(size_t)255; }

}  // namespace

extern "C" size_t ktup_eval_transd_workspace_bytes(int d, int64_t nq) {
  if (d <= 0 || nq <= 0) return 0;
  return (qw_floats(d, nq) + (size_t)nq * 4) * sizeof(float);
}

extern "C" int ktup_eval_transd_scores(const float* E, int64_t lde, const float* Ep, int64_t ldep, const float* R, int64_t ldr,
                                       const float* Rp, int64_t ldrp, int d, const float* C, int64_t ldc, int64_t n_cand,
                                       const int64_t* q, const int64_t* r, int64_t nq, int l1, int head, float* out, int64_t ldo,
                                       float* ws, void* stream) {
  const char* name = "ktup_eval_transd_scores";
  KTUP_REQUIRE(d > 0 && nq >= 0 && n_cand >= 0, "%s: bad sizes", name);
  if (nq == 0 || n_cand == 0) return KTUP_OK;
  KTUP_REQUIRE(E && Ep && R && Rp && C && q && r && out && ws, "%s: null pointer argument", name);
  KTUP_REQUIRE(ldo >= n_cand, "%s: output pitch %lld < n_cand", name, (long long)ldo);
  KTUP_REQUIRE(aligned16(ws), "%s: workspace must be 16-byte aligned", name);
  hipStream_t st = (hipStream_t)stream;
  const int dq = round4(d);
  float* QW = ws;
  float* QS = ws + qw_floats(d, nq);
  hipLaunchKernelGGL(transd_query_prep_kernel, dim3(grid_for((nq + 3) / 4)), dim3(256), 0, st, E, lde, Ep, ldep, R, ldr, Rp, ldrp, d, dq,
                     q, r, nq, head, QW, QS);
  if (int e = check_launch(name)) return e;
  if (!l1 && ktup::opt_eval_mc()) {
    const McArgs m{QW, QS, C, ldc, nq, n_cand, out, ldo};
    const int rc = transd_l2_mc(m, d, dq, st, name);
    if (rc != 1) return rc;
  }
  PairArgs a{};
  a.C = C; a.ldc = ldc; a.n_cand = n_cand; a.QW = QW; a.nq = nq; a.d = d; a.dq = dq; a.out = out; a.ldo = ldo;
  a.cvec = (d % 4 == 0) && aligned16(C) && (ldc % 4 == 0);
  return launch_pairs(a, l1, st, name);
}

extern "C" size_t ktup_eval_kg_ranks_transd_workspace_bytes(int d, int64_t n_cand, int64_t chunk) {
  if (d <= 0 || n_cand <= 0 || chunk <= 0) return 0;
  return 2 * score_bytes(chunk, n_cand) + ktup_eval_transd_workspace_bytes(d, chunk);
}

extern "C" int ktup_eval_kg_ranks_transd(const float* E, int64_t lde, const float* Ep, int64_t ldep, const float* R, int64_t ldr,
                                         const float* Rp, int64_t ldrp, int d, const float* C, int64_t ldc, int64_t n_cand,
                                         const int64_t* q, const int64_t* r, int64_t nq, int l1, int head, int descending,
                                         const int64_t* filt_off, const int32_t* filt_ids, const int64_t* gold_off,
                                         const int32_t* gold_ids, int32_t* ranks, int64_t chunk, void* ws, void* stream) {
  const char* name = "ktup_eval_kg_ranks_transd";
  KTUP_REQUIRE(nq >= 0 && n_cand > 0 && chunk > 0 && d > 0, "%s: bad sizes", name);
  if (nq == 0) return KTUP_OK;
  KTUP_REQUIRE(E && Ep && R && Rp && C && q && r && gold_off && gold_ids && ranks && ws, "%s: null pointer argument", name);
  KTUP_REQUIRE((filt_off == nullptr) || filt_ids, "%s: filter offsets without ids", name);
  KTUP_REQUIRE(aligned16(ws), "%s: workspace must be 16-byte aligned", name);
  hipStream_t st = (hipStream_t)stream;
  const size_t sb = score_bytes(chunk, n_cand) / sizeof(float);
  float* scores2 = reinterpret_cast<float*>(ws);
  float* qws = scores2 + 2 * sb;
  // The key-side scratch is rewritten per chunk.  With the side stream only the RANK kernel of a chunk runs there; the prep and score
  // kernels of all chunks stay in order on `st`, so the scratch is never rewritten while a score kernel reads it.
  hipStream_t side = (nq > chunk && events_ok()) ? ktup::fork_side(st) : nullptr;
  int64_t c = 0;
  for (int64_t c0 = 0; c0 < nq; c0 += chunk, ++c) {
    const int64_t nb = nq - c0 < chunk ? nq - c0 : chunk;
    const int b = (int)(c & 1);
    float* out = scores2 + (side ? b * sb : 0);
    if (side && c >= 2 && hipStreamWaitEvent(st, g_ev.done[b], 0) != hipSuccess) return ktup::check_launch(name);   // ranks(c - 2) has read this buffer
    int rc = ktup_eval_transd_scores(E, lde, Ep, ldep, R, ldr, Rp, ldrp, d, C, ldc, n_cand, q + c0, r + c0, nb, l1, head, out, n_cand, qws, st);
    if (rc != KTUP_OK) { ktup::join_side(st, side); return rc; }
    hipStream_t rs = st;
    if (side) {
      if (hipEventRecord(g_ev.ready[b], st) != hipSuccess || hipStreamWaitEvent(side, g_ev.ready[b], 0) != hipSuccess) return ktup::check_launch(name);
      rs = side;
    }
    rc = ktup_eval_gold_ranks(out, n_cand, nb, n_cand, descending, filt_off ? filt_off + c0 : nullptr, filt_ids, gold_off + c0, gold_ids, ranks, rs);
    if (rc != KTUP_OK) { ktup::join_side(st, side); return rc; }
    if (side && hipEventRecord(g_ev.done[b], side) != hipSuccess) return ktup::check_launch(name);
  }
  ktup::join_side(st, side);                   // the caller's stream continues after the last rank kernel
  return KTUP_OK;
}

// ---- the pass without the score matrix.  Declined (KTUP_ERR_UNSUPPORTED before any HIP call; the caller keeps the chunked route):
// rows too wide for the pair kernels' LDS stage (round4(d) > 640: the chunked route declines them too), more than 65535 x 64 keys
// in one call, 2^31 or more candidates.
extern "C" int ktup_eval_kg_ranks_transd_fused_supported(int d, int l1, int64_t max_golds) {
  (void)l1; (void)max_golds;      // (any distance; golds beyond the first four of a key: further sweep launches / the pair form's loop)
  return d > 0 && pairs_lds(round4(d)) <= 160 * 1024;
}

extern "C" size_t ktup_eval_kg_ranks_transd_fused_workspace_bytes(int d, int64_t nq, int64_t n_gold, int64_t n_filt, int64_t n_cand) {
  if (d <= 0 || nq <= 0 || n_cand <= 0) return 0;
  // QW | QS | gscore | counts | fscore | cnorm: nothing in nq x n_cand
  return pad256(ktup_eval_transd_workspace_bytes(d, nq)) + 2 * pad256((size_t)(n_gold > 0 ? n_gold : 1) * 4) +
         pad256((size_t)(n_filt > 0 ? n_filt : 1) * 4) + pad256((size_t)n_cand * 4);
}

extern "C" int ktup_eval_kg_ranks_transd_fused(const float* E, int64_t lde, const float* Ep, int64_t ldep, const float* R, int64_t ldr,
                                               const float* Rp, int64_t ldrp, int d, const float* C, int64_t ldc, int64_t n_cand,
                                               const int64_t* q, const int64_t* r, int64_t nq, int l1, int head, int descending,
                                               const int64_t* filt_off, const int32_t* filt_ids, int64_t n_filt, const int64_t* gold_off,
                                               const int32_t* gold_ids, int64_t n_gold, int64_t max_golds, int32_t* ranks, void* ws,
                                               void* stream) {
  const char* name = "ktup_eval_kg_ranks_transd_fused";
  if (!ktup_eval_kg_ranks_transd_fused_supported(d, l1, max_golds))
    return set_error(KTUP_ERR_UNSUPPORTED, "%s: embedding_size %d does not fit the pair kernels' LDS stage", name, d);
  if ((nq + 63) / 64 > 65535 || n_cand >= (1ll << 31))
    return set_error(KTUP_ERR_UNSUPPORTED, "%s: sizes out of range for one sweep (%lld keys, %lld candidates)", name, (long long)nq, (long long)n_cand);
  KTUP_REQUIRE(nq >= 0 && n_cand > 0 && n_gold >= 0 && n_filt >= 0 && max_golds >= 0, "%s: bad sizes", name);
  if (nq == 0 || n_gold == 0) return KTUP_OK;
  KTUP_REQUIRE(E && Ep && R && Rp && C && q && r && gold_off && gold_ids && ranks && ws, "%s: null pointer argument", name);
  KTUP_REQUIRE((filt_off == nullptr) || filt_ids, "%s: filter offsets without ids", name);
  KTUP_REQUIRE(aligned16(ws), "%s: workspace must be 16-byte aligned", name);
  hipStream_t st = (hipStream_t)stream;
  const int dq = round4(d);
  char* p = reinterpret_cast<char*>(ws);
  float* QW = reinterpret_cast<float*>(p);
  float* QS = QW + qw_floats(d, nq); p += pad256(ktup_eval_transd_workspace_bytes(d, nq));
  float* gscore = reinterpret_cast<float*>(p); p += pad256((size_t)n_gold * 4);
  int32_t* counts = reinterpret_cast<int32_t*>(p); p += pad256((size_t)n_gold * 4);
  float* fscore = reinterpret_cast<float*>(p); p += pad256((size_t)(n_filt > 0 ? n_filt : 1) * 4);
  float* cnorm = reinterpret_cast<float*>(p);
  hipLaunchKernelGGL(transd_query_prep_kernel, dim3(grid_for((nq + 3) / 4)), dim3(256), 0, st, E, lde, Ep, ldep, R, ldr, Rp, ldrp, d, dq,
                     q, r, nq, head, QW, QS);
  if (int e = check_launch(name)) return e;
  int rc = 1;
  if (dq == d && pass_mc_covers(d, l1, C, ldc, n_cand)) {
    PassArgs a{};
    a.QW = QW; a.QS = QS; a.C = C; a.ldc = ldc; a.nq = nq; a.n_cand = n_cand; a.descending = descending;
    a.gold_off = gold_off; a.gold_ids = gold_ids; a.gscore = gscore; a.filt_off = filt_off; a.filt_ids = filt_ids; a.fscore = fscore;
    a.counts = counts; a.cnorm = cnorm;
    switch (d) {
      case 20: rc = run_pass_mc<PGeom<5>>(a, n_gold, max_golds, cnorm, st, name); break;
      case 36: rc = run_pass_mc<PGeom<9>>(a, n_gold, max_golds, cnorm, st, name); break;
      case 64: rc = run_pass_mc<PGeom<16>>(a, n_gold, max_golds, cnorm, st, name); break;
      case 100: rc = run_pass_mc<PGeom<25>>(a, n_gold, max_golds, cnorm, st, name); break;
      case 128: rc = run_pass_mc<PGeom<32>>(a, n_gold, max_golds, cnorm, st, name); break;
      default: break;
    }
  }
  if (rc == 1) {
    // L1, the other widths, unaligned or odd-pitch candidate tables, option eval_mc = 0: the pair kernel's list and COUNT forms
    hipLaunchKernelGGL(transd_pass_init_kernel, dim3(grid_for((n_gold + 255) / 256, 2048)), dim3(256), 0, st, counts, n_gold, C, ldc, 0,
                       (int64_t)0, cnorm);
    PairArgs a{};
    a.C = C; a.ldc = ldc; a.n_cand = n_cand; a.QW = QW; a.nq = nq; a.d = d; a.dq = dq;
    a.cvec = (d % 4 == 0) && aligned16(C) && (ldc % 4 == 0);
    a.descending = descending; a.gold_off = gold_off; a.gold_ids = gold_ids; a.gscore = gscore;
    a.filt_off = filt_off; a.filt_ids = filt_ids; a.fscore = fscore; a.counts = counts;
    rc = launch_pairs_count(a, l1, st, name);
  }
  if (rc != KTUP_OK) return rc;
  return kg_rank_finalize(gold_off, gold_ids, gscore, filt_off, filt_ids, fscore, counts, ranks, nq, n_cand, n_gold, descending, st, name);
}
