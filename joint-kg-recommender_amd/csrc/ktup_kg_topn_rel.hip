// Link prediction as lists for the models whose CANDIDATE side depends on the key's relation: TransR / CKE (transR.py:80-128,
// CKE.py:155-203: every entity is projected by the relation's matrix) and TransD (transD.py:78-134: every entity is projected with the
// query's row a along the relation's row b).  The filtered top-n ENTITIES of every key (q, r) in one sweep that never writes the
// (keys x entities) matrix.  See include/ktup_hip.h, ktup_eval_kg_topk_rel; ktup_kg_topn.hip is the pass of TransE / TransH.
//
// The sweep is ktup_sweep_pass.h's, unchanged: a workgroup stages ONE stream of candidate rows for its 64 keys, so those 64 keys
// must share a relation.  This file adds
//   * the buckets: keys are counted per relation (atomics, any number of workgroups), every relation with keys claims a run of whole
//     64-key blocks from one counter, and the keys are scattered into that padded POSITION space: pos2key[] (a pad position points at
//     the first key of its block; its list is never read), key2pos[], blk_rel[].  The host cannot know the distribution: workspace and
//     grid are sized for nq / 64 + min(n_rel, nq) blocks, and a workgroup past the used count leaves before the pass (a uniform test).
//     Which position a key gets depends on the order of the atomics; its list does not: it is a function of the key alone;
//   * the filter bits by position (sweep_filter_bits' layout, the CSR list of pos2key[pos]) and, after sweep_merge, the move of the
//     lists from position order to key order;
//   * the scorer.  Its row(c) and spare(c) read the block's relation rho.
//       TransR: the entity table is projected once per call, P[rho][e] = M_rho e (rows of round4(d) floats, zero tail: always whole,
//         aligned float4, so only the vector stage loads exist), with |M_rho e|^2 beside it.  A block then runs TransE's arithmetic
//         against slice rho with c = M_r E[q] +- R[r] from kg_query_prep (model 2): squared L2 = |c|^2 - 2 c.e' + |e'|^2 on
//         v_mfma_f32_16x16x4_f32, |e'|^2 in the spare slot; L1 on the VALU against a wave's 16 c rows in LDS.
//       TransD: z = c - e - (a.e) b with a = Ep[q] the QUERY's row, b = Rp[rho] the block's.  t = b.e depends on (rho, e) only: an
//         n_rel x n_ent table built once per call rides in the spare slot beside |e|^2.  Squared L2 =
//         |c|^2 - 2 c.e + |e|^2 - 2 s (b.c - t) + s^2 |b|^2 with s = a.e: two MFMA chains against the staged tile, c and a as register
//         operands (TransH's shape, and its stage / workgroups-per-CU rules); the s terms are folded into the accumulator so that
//         score() is TransE's expression.  L1: s on the matrix cores, then sum |c_k - e_k - s b_k| on the VALU, the c rows and the
//         block's one b row in LDS.
// A score is a function of the (key, candidate) pair's own chains: the same bits at every list width, split count and key order.
// Counters are cleared by a kernel (no memset node: DESIGN section 8).
#include "ktup_pref_geom.h"
#include "ktup_sweep_pass.h"

using namespace ktup;

namespace ktup {
namespace {

constexpr int REL_MAX = 16384;

inline int round4(int d) { return (d + 3) / 4 * 4; }
inline size_t up16(size_t x) { return (x + 15) & ~(size_t)15; }
inline int64_t rel_blocks_max(int64_t nq, int64_t n_rel) { return nq / 64 + (n_rel < nq ? n_rel : nq); }

// ---- the buckets ----------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void rel_clear_kernel(int32_t* __restrict__ p, int64_t n) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) p[i] = 0;
}

KTUP_DEV int rel_of(const int64_t* r, int64_t i, int n_rel) {              // (an id outside the table lands in a bucket that exists)
  const int64_t v = r[i];
  return (int)(v < 0 ? 0 : v >= n_rel ? n_rel - 1 : v);
}

__global__ __launch_bounds__(256) void rel_count_kernel(const int64_t* __restrict__ r, int64_t nq, int n_rel, int32_t* __restrict__ cnt) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < nq; i += (int64_t)gridDim.x * 256) atomicAdd(cnt + rel_of(r, i, n_rel), 1);
}

// every relation with keys claims ceil(cnt / 64) consecutive blocks
__global__ __launch_bounds__(256) void rel_runs_kernel(const int32_t* __restrict__ cnt, int n_rel, int32_t* __restrict__ start,
                                                       int32_t* __restrict__ nblk, int32_t* __restrict__ blk_rel, int64_t nblk_max) {
  for (int rho = blockIdx.x * 256 + threadIdx.x; rho < n_rel; rho += gridDim.x * 256) {
    const int nb = (cnt[rho] + 63) >> 6;
    if (!nb) continue;
    const int s = atomicAdd(nblk, nb);
    start[rho] = s;
    for (int b = 0; b < nb && s + b < nblk_max; ++b) blk_rel[s + b] = rho;
  }
}

__global__ __launch_bounds__(256) void rel_scatter_kernel(const int64_t* __restrict__ r, int64_t nq, int n_rel,
                                                          const int32_t* __restrict__ start, int32_t* __restrict__ fill,
                                                          int64_t* __restrict__ pos2key, int64_t* __restrict__ key2pos, int64_t nqp) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < nq; i += (int64_t)gridDim.x * 256) {
    const int rho = rel_of(r, i, n_rel);
    const int64_t pos = (int64_t)start[rho] * 64 + atomicAdd(fill + rho, 1);
    key2pos[i] = pos;
    if (pos < nqp) pos2key[pos] = i;
  }
}

// pad positions of the used blocks -> the first key of their block (position 0 of a block always holds a key); the filter bits of
// the used positions <- 0
__global__ __launch_bounds__(256) void rel_pad_kernel(const int32_t* __restrict__ cnt, const int32_t* __restrict__ start,
                                                      const int32_t* __restrict__ nblk, const int32_t* __restrict__ blk_rel,
                                                      int64_t* __restrict__ pos2key, uint32_t* __restrict__ bm, int64_t words) {
  const int64_t npos = (int64_t)*nblk * 64;
  for (int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x; p < npos; p += (int64_t)gridDim.x * 256) {
    const int rho = blk_rel[p >> 6];
    if (p - (int64_t)start[rho] * 64 >= cnt[rho]) pos2key[p] = pos2key[p & ~(int64_t)63];
  }
  if (bm) {
    const int64_t nw = npos * words;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < nw; i += (int64_t)gridDim.x * 256) bm[i] = 0u;
  }
}

// sweep_filter_bits_kernel by position: one wave per used position, the CSR list of its key
__global__ __launch_bounds__(256) void rel_filter_bits_kernel(const int64_t* __restrict__ off, const int32_t* __restrict__ ids,
                                                              const int32_t* __restrict__ nblk, const int64_t* __restrict__ pos2key,
                                                              int64_t n, uint32_t* __restrict__ bm, int64_t words) {
  const int lane = threadIdx.x & 63;
  const int64_t npos = (int64_t)*nblk * 64;
  for (int64_t p = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); p < npos; p += (int64_t)gridDim.x * 4) {
    const int64_t b = pos2key[p];
    const int64_t f1 = off[b + 1];
    for (int64_t f = off[b] + lane; f < f1; f += 64) {
      const int64_t id = ids[f];
      if (id >= 0 && id < n) atomicOr(bm + p * words + (id >> 5), 1u << (id & 31));
    }
  }
}

// the merged lists, position order -> key order
__global__ __launch_bounds__(256) void rel_unscatter_kernel(const int64_t* __restrict__ key2pos, int64_t nq, int topn,
                                                            const int32_t* __restrict__ pid, const float* __restrict__ psc,
                                                            int32_t* __restrict__ top_ids, float* __restrict__ top_scores) {
  const int64_t n = nq * topn;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
    const int64_t b = i / topn;
    const int64_t src = key2pos[b] * topn + (i - b * topn);
    top_ids[i] = pid[src];
    if (top_scores) top_scores[i] = psc[src];
  }
}

// ---- what a call computes once ----------------------------------------------------------------------------------------------------
// TransR: P[rho][e][dq] = M_rho e (zero tail) and PN[rho][e] = |M_rho e|^2 (misc.py:29-33; transr_project_kernel of ktup_eval.hip with
// the norm).  Workgroup = (64-entity tile, relation); lane <-> entity, the waves split the output coordinates; M rows are wave-uniform.
constexpr int PT = 64;
__global__ __launch_bounds__(256) void rel_transr_project_kernel(const float* __restrict__ E, int64_t lde, const float* __restrict__ M,
                                                                 int64_t ldm, int d, int dq, int64_t n_ent, int evec,
                                                                 float* __restrict__ P, float* __restrict__ PN) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  v4* cand = reinterpret_cast<v4*>(smem);                                  // [dq / 4][PT]
  float* part = reinterpret_cast<float*>(cand + (dq / 4) * PT);            // [4][PT]
  const int t = threadIdx.x, lane = t & 63;
  const int w = __builtin_amdgcn_readfirstlane(t >> 6);
  const int nch4 = dq / 4;
  const int64_t j0 = (int64_t)blockIdx.x * PT;
  const int rho = blockIdx.y;
  for (int idx = t; idx < nch4 * PT; idx += 256) {
    const int j = idx & (PT - 1), c = idx >> 6;
    const float* row = E + min(j0 + j, n_ent - 1) * lde;
    v4 v;
    if (evec) {
      v = *reinterpret_cast<const v4*>(row + 4 * c);
    } else {
#pragma unroll
      for (int k = 0; k < 4; ++k) v[k] = 4 * c + k < d ? row[4 * c + k] : 0.f;
    }
    cand[c * PT + j] = v;
  }
  __syncthreads();
  const float* Mr = M + (int64_t)rho * ldm;
  const bool live = j0 + lane < n_ent;
  float* outrow = P + ((int64_t)rho * n_ent + min(j0 + lane, n_ent - 1)) * dq;
  float nrm = 0.f;
  for (int i = w; i < dq; i += 4) {
    float acc = 0.f;
    if (i < d) {
      const float* mrow = Mr + (int64_t)i * d;
      for (int c = 0; c < nch4; ++c) {
        const v4 e4 = cand[c * PT + lane];
#pragma unroll
        for (int k = 0; k < 4; ++k)
          if (4 * c + k < d) acc = fmaf(mrow[4 * c + k], e4[k], acc);
      }
    }
    nrm = fmaf(acc, acc, nrm);
    if (live) outrow[i] = acc;
  }
  part[w * PT + lane] = nrm;
  __syncthreads();
  if (w == 0 && live && PN) PN[(int64_t)rho * n_ent + j0 + lane] = (part[lane] + part[PT + lane]) + (part[2 * PT + lane] + part[3 * PT + lane]);
}

// TransD, squared L2: T[rho][e] = Rp[rho] . E[e] and |E[e]|^2 (written by relation 0's workgroups).  16 lanes per (rho, e).
__global__ __launch_bounds__(256) void rel_transd_tables_kernel(const float* __restrict__ E, int64_t lde, const float* __restrict__ Rp,
                                                                int64_t ldrp, int d, int64_t n_ent, float* __restrict__ T,
                                                                float* __restrict__ enorm) {
  const int l = threadIdx.x & 15;
  const int rho = blockIdx.y;
  const float* b = Rp + (int64_t)rho * ldrp;
  for (int64_t c = (int64_t)blockIdx.x * 16 + (threadIdx.x >> 4); c < n_ent; c += (int64_t)gridDim.x * 16) {
    const float* row = E + c * lde;
    float t = 0.f, s = 0.f;
    for (int k = l; k < d; k += 16) {
      t = fmaf(b[k], row[k], t);
      s = fmaf(row[k], row[k], s);
    }
    t = group_sum<16>(t);
    s = group_sum<16>(s);
    if (l == 0) {
      T[(int64_t)rho * n_ent + c] = t;
      if (rho == 0) enorm[c] = s;
    }
  }
}

// TransD, per key (transd_query_prep_kernel's rows without the b row, which is the block's): QW[i] = [c | a] (2 x dq floats, zero
// tail), QS[i] = {b.c, |b|^2}.  One wave per key.
__global__ __launch_bounds__(256) void rel_transd_keys_kernel(const float* __restrict__ E, int64_t lde, const float* __restrict__ Ep,
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
    float* out = QW + i * 2 * dq;
    float dot = 0.f;
    for (int k = lane; k < d; k += 64) dot = fmaf(e[k], a[k], dot);
    dot = group_sum<64>(dot);
    float bc = 0.f, bb = 0.f;
    for (int k = lane; k < dq; k += 64) {
      float c = 0.f, av = 0.f, bv = 0.f;
      if (k < d) { av = a[k]; bv = b[k]; c = fmaf(dot, bv, e[k]) + sgn * rel[k]; }
      out[k] = c; out[dq + k] = av;
      bc = fmaf(bv, c, bc); bb = fmaf(bv, bv, bb);
    }
    bc = group_sum<64>(bc); bb = group_sum<64>(bb);
    if (lane == 0) { QS[2 * i] = bc; QS[2 * i + 1] = bb; }
  }
}

// ---- the scorer ---------------------------------------------------------------------------------------------------------------------
struct RelTopnArgs {
  SweepArgs sw;                         // u_ids = pos2key, nq = the padded positions
  const int32_t* nblk;                  // blocks in use
  const int32_t* blk_rel;               // the relation of each
  const float* QW; int qs, dq;          // [nq][qs] in KEY order: c at 0, TransD's a at dq
  const float* QS;                      // TransD [nq][2]: b.c, |b|^2
  const float* C; int64_t ldc, slice;   // candidate rows: TransR P (slice = n_ent * dq floats per relation), TransD E (slice 0)
  const float* N; int64_t nslice;       // squared L2: |e'|^2, TransR [n_rel][n_ent] (nslice = n_ent), TransD [n_ent] (0); NULL under L1
  const float* T;                       // TransD, squared L2: [n_rel][n_ent] b.e
  const float* Rp; int64_t ldrp;        // TransD, L1: the b rows
};

// NSUB dot products of a stage on v_mfma_f32_16x16x4_f32, k ascending (sweep_tile_dot for any stage size)
template <int KS, int NSUB>
KTUP_DEV void rel_tile_dot(const float (&av)[KS], const v4* eb, int kq, v4 (&acc)[NSUB]) {
  constexpr int ROW4 = SweepGeom<KS>::ROW4;
  const float* rb = reinterpret_cast<const float*>(eb) + kq;               // lane (kq, candidate j): element kq of every k quad
#pragma unroll
  for (int s = 0; s < KS; ++s) {
#pragma unroll
    for (int t = 0; t < NSUB; ++t) acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[s], rb[t * 16 * ROW4 * 4 + 4 * s], acc[t], 0, 0, 0);
  }
}

// The sweep ranks s = -distance descending: ascending distance, ties -> lower entity.  D: TransD (else TransR on projected rows).
template <int KS, bool L1, bool D, int STC = 0>
struct RelScorer {
  using G = SweepGeom<KS, STC>;
  // L1: a wave's 16 c rows in LDS for the whole pass, [16][CROW4] float4, and for TransD the block's b row behind them, [KS] float4
  static constexpr int CROW4 = KS | 1;
  static constexpr size_t CW = !L1 ? 0 : (size_t)(16 * CROW4 + (D ? KS : 0)) * 16;
  static constexpr size_t LDS = 4 * CW;
  const RelTopnArgs& a;
  int64_t rho;                                                            // the block's relation
  float cn[4] = {0.f, 0.f, 0.f, 0.f};                                     // squared L2: |c|^2 of the keys of this lane's accumulator rows
  float bc[4] = {0.f, 0.f, 0.f, 0.f};                                     // TransD, squared L2: b.c of those keys
  float hbb[4] = {0.f, 0.f, 0.f, 0.f};                                    //   ... and -|b|^2 / 2
  const v4* cw = nullptr;                                                 // L1: the c rows of those four keys, [4][CROW4]
  const v4* bw = nullptr;                                                 // L1, TransD: the b row
  float wv[D ? KS : 1];                                                   // TransD: the A operand of a.e -- element 4 s + kq of key j's a row
  KTUP_DEV float query(int64_t u, int k) const { return a.QW[u * a.qs + k]; }
  KTUP_DEV void hold(const float (&av)[KS], char* smem, int64_t u0, const bool (&in)[4], int kq, int j) {
    if constexpr (D) {
      const bool ok = u0 + j < a.sw.nq;
      const float* w = a.QW + a.sw.u_ids[ok ? u0 + j : (int64_t)0] * a.qs + a.dq;
#pragma unroll
      for (int s = 0; s < KS; ++s) wv[s] = w[min(4 * s + kq, a.sw.d - 1)];
#pragma unroll
      for (int s = 0; s < KS; ++s) wv[s] = (ok && 4 * s + kq < a.sw.d) ? wv[s] : 0.f;
    }
    if constexpr (L1) {
      float* cwf = reinterpret_cast<float*>(smem + (size_t)__builtin_amdgcn_readfirstlane(threadIdx.x >> 6) * CW);   // [16][CROW4] float4
#pragma unroll
      for (int s = 0; s < KS; ++s) cwf[(j * CROW4 + s) * 4 + kq] = av[s];
      cw = reinterpret_cast<const v4*>(cwf) + 4 * kq * CROW4;
      if constexpr (D) {
        float* bf = cwf + 16 * CROW4 * 4;                                  // [KS] float4, this wave's copy
        const float* b = a.Rp + rho * a.ldrp;
        for (int k = (int)(threadIdx.x & 63); k < 4 * KS; k += 64) bf[k] = k < a.sw.d ? b[k] : 0.f;
        bw = reinterpret_cast<const v4*>(bf);
      }
    } else {
      float cnj = 0.f;
#pragma unroll
      for (int s = 0; s < KS; ++s) cnj = fmaf(av[s], av[s], cnj);
      cnj += __shfl_xor(cnj, 16, 64);
      cnj += __shfl_xor(cnj, 32, 64);                                     // |c|^2 of key j on every lane (., j)
#pragma unroll
      for (int reg = 0; reg < 4; ++reg) cn[reg] = __shfl(cnj, 4 * kq + reg, 64);
      if constexpr (D) {
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) {
          const int64_t p = a.sw.u_ids[in[reg] ? u0 + 4 * kq + reg : (int64_t)0];
          const float x = a.QS[2 * p], y = a.QS[2 * p + 1];
          bc[reg] = in[reg] ? x : 0.f;
          hbb[reg] = in[reg] ? -0.5f * y : 0.f;
        }
      }
    }
  }
  KTUP_DEV const float* row(int64_t c, bool& live) const {
    live = true;
    return a.C + rho * a.slice + c * a.ldc;
  }
  KTUP_DEV v4 spare(int64_t c, bool) const {
    return (v4){a.N ? a.N[rho * a.nslice + c] : 0.f, 1.f, (D && a.T) ? a.T[rho * a.sw.n + c] : 0.f, 0.f};
  }
  // acc[t][reg] of key 4 kq + reg x candidate 16 t + j.  Squared L2: c.e, for TransD plus s (b.c - t) - s^2 |b|^2 / 2, so that score()
  // is TransE's expression for both.  L1: the distance itself.
  KTUP_DEV void tile_math(const float (&av)[KS], const v4* eb, int kq, v4 (&acc)[G::NSUB]) const {
    v4 se[G::NSUB];
    if constexpr (D) {
#pragma unroll
      for (int t = 0; t < G::NSUB; ++t) se[t] = (v4){0.f, 0.f, 0.f, 0.f};
      rel_tile_dot<KS, G::NSUB>(wv, eb, kq, se);
    }
    if constexpr (L1) {
#pragma unroll 2
      for (int s = 0; s < KS; ++s) {
        v4 cq[4], bq = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) cq[reg] = cw[reg * CROW4 + s];
        if constexpr (D) bq = bw[s];
#pragma unroll
        for (int t = 0; t < G::NSUB; ++t) {
          const v4 e = eb[t * 16 * G::ROW4 + s];
#pragma unroll
          for (int reg = 0; reg < 4; ++reg) {
            v4 z = cq[reg] - e;
            if constexpr (D) {
#pragma unroll
              for (int q = 0; q < 4; ++q) z[q] = fmaf(-se[t][reg], bq[q], z[q]);
            }
            acc[t][reg] += (fabsf(z[0]) + fabsf(z[1])) + (fabsf(z[2]) + fabsf(z[3]));
          }
        }
      }
    } else {
      rel_tile_dot<KS, G::NSUB>(av, eb, kq, acc);
      if constexpr (D) {
#pragma unroll
        for (int t = 0; t < G::NSUB; ++t) {
          const float tt = eb[t * 16 * G::ROW4 + KS][2];                  // b.e of candidate 16 t + j
#pragma unroll
          for (int reg = 0; reg < 4; ++reg) {
            const float x = se[t][reg];
            acc[t][reg] = fmaf(x, fmaf(hbb[reg], x, bc[reg] - tt), acc[t][reg]);
          }
        }
      }
    }
  }
  KTUP_DEV v4 staged(const v4* slot) const { return *slot; }
  KTUP_DEV bool live(const v4& spare) const { return spare[1] != 0.f; }
  KTUP_DEV float score(float acc, int reg, const v4& spare) const {
    return -(L1 ? acc : __fadd_rn(fmaf(-2.f, acc, cn[reg]), spare[0]));    // |c|^2 - 2 acc + |e|^2
  }
};

// The stage and workgroups-per-CU rules of ktup_kg_topn.hip (kg_topn_stage, kg_topn_wgs) with TransD in TransH's place: L1 beyond
// d = 192 under the wide lists stages ONE 16-candidate tile; TransD with squared L2 holds two register operands -- at KS = 16 and 25
// the stage is halved, from KS = 32 on (and at KS = 25 with the element-wise stage loads, which hold more addresses) the kernel is
// compiled for one workgroup per CU.
constexpr int rel_topn_stage(int ks, bool l1, bool dd, int seg) {
  return seg > 1 && l1 && ks > 48 ? 16 : dd && !l1 && (ks == 16 || ks == 25) ? 32 : 0;
}

template <int KS, bool L1, bool D, int SEG>
constexpr size_t rel_topn_lds() {
  constexpr int STC = rel_topn_stage(KS, L1, D, SEG);
  return SweepGeom<KS, STC>::lds(RelScorer<KS, L1, D, STC>::LDS, SEG);
}

template <int KS, bool VEC, bool L1, bool D, int SEG>
constexpr int rel_topn_wgs() {
  return D && !L1 && (KS >= 32 || (KS == 25 && !VEC)) ? 1 : sweep_wide_wgs(rel_topn_lds<KS, L1, D, SEG>());
}

template <int KS, bool VEC, bool L1, bool D, int SEG>
__global__ __launch_bounds__(256, (rel_topn_wgs<KS, VEC, L1, D, SEG>())) void kg_topn_rel_kernel(RelTopnArgs a) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int blk = (int)(blockIdx.x / (unsigned)a.sw.nsplit);
  if (blk >= *a.nblk) return;                                              // (uniform: the grid is sized for the worst distribution)
  constexpr int STC = rel_topn_stage(KS, L1, D, SEG);
  RelScorer<KS, L1, D, STC> sc{a, (int64_t)a.blk_rel[blk]};
  sweep_pass<KS, VEC, SEG, STC>(a.sw, sc, smem);
}

template <int KS, bool L1, bool D, int SEG>
int launch_kg_topn_rel(const RelTopnArgs& a, hipStream_t st, const char* name) {
  constexpr size_t lds = rel_topn_lds<KS, L1, D, SEG>();
  if constexpr (D) {
    if (!a.sw.vec) return sweep_launch<lds>(kg_topn_rel_kernel<KS, false, L1, true, SEG>, a, a.sw, st, name);
  }
  return sweep_launch<lds>(kg_topn_rel_kernel<KS, true, L1, D, SEG>, a, a.sw, st, name);
}

inline bool rel_covers(int model, int d, int topn) {
  return (model == KTUP_KG_TRANSR || model == KTUP_KG_TRANSD) && d >= 1 && d <= 256 && topn >= 1 && topn <= TOPN_WIDE_MAX;
}

// the workspace behind the sweep's: counters (cnt | fill | nblk) | start | blk_rel | pos2key | key2pos | QW | QS | the lists in
// position order (ids | scores) | the tables of the call
struct RelLayout {
  int64_t nblk_max, nqp;
  size_t sweep, ctr, start, blk_rel, pos2key, key2pos, qw, qs, pid, psc, tab, total;
};
inline RelLayout rel_layout(int model, int d, int64_t nq, int64_t n_ent, int64_t n_rel, int topn, int nsplit) {
  RelLayout L{};
  const bool dd = model == KTUP_KG_TRANSD;
  const size_t dq = (size_t)round4(d);
  L.nblk_max = rel_blocks_max(nq, n_rel);
  L.nqp = L.nblk_max * 64;
  L.sweep = sweep_workspace_bytes(L.nqp, n_ent, topn, TOPN_WIDE_MAX, nsplit, dd ? 1 : 0);
  size_t o = up16(L.sweep);
  auto take = [&](size_t bytes) { const size_t at = o; o += up16(bytes); return at; };
  L.ctr = take((size_t)(2 * n_rel + 4) * sizeof(int32_t));
  L.start = take((size_t)n_rel * sizeof(int32_t));
  L.blk_rel = take((size_t)L.nblk_max * sizeof(int32_t));
  L.pos2key = take((size_t)L.nqp * sizeof(int64_t));
  L.key2pos = take((size_t)nq * sizeof(int64_t));
  L.qw = take((size_t)nq * (dd ? 2 : 3) * dq * sizeof(float));
  L.qs = take((size_t)nq * 2 * sizeof(float));
  L.pid = take((size_t)L.nqp * topn * sizeof(int32_t));
  L.psc = take((size_t)L.nqp * topn * sizeof(float));
  L.tab = take(dd ? (size_t)n_rel * n_ent * sizeof(float) : (size_t)n_rel * n_ent * (dq + 1) * sizeof(float));
  L.total = o + 16;
  return L;
}

}  // namespace
}  // namespace ktup

extern "C" int ktup_eval_kg_topk_rel_supported(int model, int d, int l1, int topn) {
  (void)l1;
  return rel_covers(model, d, topn) ? 1 : 0;
}

extern "C" size_t ktup_eval_kg_topk_rel_workspace_bytes(int model, int d, int64_t nq, int64_t n_ent, int64_t n_rel, int topn, int nsplit) {
  if (!rel_covers(model, d, topn) || nq < 1 || n_ent < 1 || n_ent >= ((int64_t)1 << 31) || n_rel < 1 || n_rel > REL_MAX || nsplit < 0) return 0;
  const RelLayout L = rel_layout(model, d, nq, n_ent, n_rel, topn, nsplit);
  return L.sweep ? L.total : 0;
}

extern "C" int ktup_eval_kg_topk_rel(int model, const float* E, int64_t lde, const float* R, int64_t ldr, const float* A, int64_t lda,
                                     const float* B, int64_t ldb, int64_t n_rel, int d, int64_t n_ent, const int64_t* q, const int64_t* r,
                                     int64_t nq, int l1, int head, const int64_t* filt_off, const int32_t* filt_ids, int topn, int nsplit,
                                     int32_t* top_ids, float* top_scores, void* ws, void* stream) {
  const char* name = "ktup_eval_kg_topk_rel";
  if (model != KTUP_KG_TRANSR && model != KTUP_KG_TRANSD)
    return set_error(KTUP_ERR_UNSUPPORTED, "%s: model %d is neither KTUP_KG_TRANSR nor KTUP_KG_TRANSD", name, model);
  const bool dd = model == KTUP_KG_TRANSD;
  KTUP_REQUIRE(E, "%s: null entity table E", name);
  KTUP_REQUIRE(R, "%s: null relation table R", name);
  KTUP_REQUIRE(A, "%s: null table A (%s)", name, dd ? "KTUP_KG_TRANSD: the entity projection rows Ep" : "KTUP_KG_TRANSR: the matrices M");
  KTUP_REQUIRE(!dd || B, "%s: null table B (KTUP_KG_TRANSD: the relation projection rows Rp)", name);
  KTUP_REQUIRE(q && r, "%s: null key ids (q, r)", name);
  KTUP_REQUIRE(top_ids, "%s: null output top_ids", name);
  KTUP_REQUIRE(ws, "%s: null workspace ws", name);
  KTUP_REQUIRE(d >= 1 && nq >= 0 && n_ent > 0 && n_rel > 0 && topn > 0 && nsplit >= 0,
               "%s: bad sizes (embedding_size d %d, nq %lld, n_ent %lld, n_rel %lld, topn %d, nsplit %d)", name, d, (long long)nq,
               (long long)n_ent, (long long)n_rel, topn, nsplit);
  KTUP_REQUIRE(lde >= d && ldr >= d, "%s: a row pitch (lde, ldr) is below embedding_size %d", name, d);
  if (dd) KTUP_REQUIRE(lda >= d && ldb >= d, "%s: a row pitch (lda, ldb) is below embedding_size %d", name, d);
  else KTUP_REQUIRE(lda >= (int64_t)d * d, "%s: the matrix pitch lda %lld is below embedding_size^2 = %lld", name, (long long)lda, (long long)d * d);
  KTUP_REQUIRE((filt_off == nullptr) == (filt_ids == nullptr), "%s: filt_off and filt_ids go together", name);
  KTUP_REQUIRE((reinterpret_cast<uintptr_t>(ws) & 15) == 0, "%s: the workspace ws must be 16-byte aligned", name);
  if (topn > TOPN_WIDE_MAX) return set_error(KTUP_ERR_UNSUPPORTED, "%s: topn %d > %d", name, topn, TOPN_WIDE_MAX);
  if (d > 256) return set_error(KTUP_ERR_UNSUPPORTED, "%s: embedding_size %d > 256", name, d);
  if (n_ent >= ((int64_t)1 << 31)) return set_error(KTUP_ERR_UNSUPPORTED, "%s: n_ent %lld does not fit 32-bit ids", name, (long long)n_ent);
  if (n_rel > REL_MAX) return set_error(KTUP_ERR_UNSUPPORTED, "%s: n_rel %lld > %d", name, (long long)n_rel, REL_MAX);
  if (nq == 0) return KTUP_OK;
  hipStream_t st = (hipStream_t)stream;
  const int dq = round4(d), nr = (int)n_rel;
  const RelLayout L = rel_layout(model, d, nq, n_ent, n_rel, topn, nsplit);
  char* base = reinterpret_cast<char*>(ws);
  int32_t* cnt = reinterpret_cast<int32_t*>(base + L.ctr);
  int32_t* fill = cnt + n_rel;
  int32_t* nblk = fill + n_rel;
  int32_t* start = reinterpret_cast<int32_t*>(base + L.start);
  int32_t* blk_rel = reinterpret_cast<int32_t*>(base + L.blk_rel);
  int64_t* pos2key = reinterpret_cast<int64_t*>(base + L.pos2key);
  int64_t* key2pos = reinterpret_cast<int64_t*>(base + L.key2pos);
  float* QW = reinterpret_cast<float*>(base + L.qw);
  float* QS = reinterpret_cast<float*>(base + L.qs);
  int32_t* pid = reinterpret_cast<int32_t*>(base + L.pid);
  float* psc = reinterpret_cast<float*>(base + L.psc);
  float* tab = reinterpret_cast<float*>(base + L.tab);

  RelTopnArgs a{};
  a.nblk = nblk; a.blk_rel = blk_rel; a.QW = QW; a.qs = (dd ? 2 : 3) * dq; a.dq = dq; a.QS = QS;
  a.sw.u_ids = pos2key; a.sw.nq = L.nqp; a.sw.n = n_ent; a.sw.topn = topn;
  if (dd) {
    a.C = E; a.ldc = lde; a.slice = 0; a.nslice = 0; a.Rp = B; a.ldrp = ldb;
    a.sw.d = d;
    a.sw.vec = (d % 4 == 0 && lde % 4 == 0 && aligned16(E)) ? 1 : 0;
  } else {
    a.C = tab; a.ldc = dq; a.slice = n_ent * dq; a.nslice = n_ent;
    a.sw.d = dq;                                                           // (the projected rows and kg_query_prep's c are dq wide, zero tail)
    a.sw.vec = 1;
  }
  float* en = nullptr;
  if (int rc = sweep_prepare(a.sw, nsplit, nullptr, nullptr, ws, &en, st, name)) return rc;
  uint32_t* bm = filt_off ? reinterpret_cast<uint32_t*>(a.sw.part + (size_t)a.sw.nq * a.sw.nsplit * a.sw.topn) : nullptr;

  // the buckets
  hipLaunchKernelGGL(rel_clear_kernel, dim3(grid_for((2 * n_rel + 4 + 255) / 256)), dim3(256), 0, st, cnt, 2 * n_rel + 4);
  if (int rc = check_launch(name)) return rc;
  hipLaunchKernelGGL(rel_count_kernel, dim3(grid_for((nq + 255) / 256)), dim3(256), 0, st, r, nq, nr, cnt);
  if (int rc = check_launch(name)) return rc;
  hipLaunchKernelGGL(rel_runs_kernel, dim3(grid_for((n_rel + 255) / 256)), dim3(256), 0, st, cnt, nr, start, nblk, blk_rel, L.nblk_max);
  if (int rc = check_launch(name)) return rc;
  hipLaunchKernelGGL(rel_scatter_kernel, dim3(grid_for((nq + 255) / 256)), dim3(256), 0, st, r, nq, nr, start, fill, pos2key, key2pos, L.nqp);
  if (int rc = check_launch(name)) return rc;
  hipLaunchKernelGGL(rel_pad_kernel, dim3(grid_for((L.nqp * (bm ? a.sw.bm_words : 1) + 255) / 256)), dim3(256), 0, st, cnt, start, nblk,
                     blk_rel, pos2key, bm, a.sw.bm_words);
  if (int rc = check_launch(name)) return rc;
  if (bm) {
    hipLaunchKernelGGL(rel_filter_bits_kernel, dim3(grid_for((L.nqp + 3) / 4, 4096)), dim3(256), 0, st, filt_off, filt_ids, nblk, pos2key, n_ent,
                       bm, a.sw.bm_words);
    if (int rc = check_launch(name)) return rc;
    a.sw.bm = bm;
  }
  // the keys' vectors and the tables of the call
  if (dd) {
    hipLaunchKernelGGL(rel_transd_keys_kernel, dim3(grid_for((nq + 3) / 4)), dim3(256), 0, st, E, lde, A, lda, R, ldr, B, ldb, d, dq, q, r, nq,
                       head, QW, QS);
    if (int rc = check_launch(name)) return rc;
    if (!l1) {
      hipLaunchKernelGGL(rel_transd_tables_kernel, dim3((unsigned)min((n_ent + 15) / 16, (int64_t)4096), (unsigned)nr), dim3(256), 0, st, E, lde,
                         B, ldb, d, n_ent, tab, en);
      if (int rc = check_launch(name)) return rc;
      a.N = en; a.T = tab;
    }
  } else {
    if (int rc = kg_query_prep(2, E, lde, R, ldr, A, lda, d, q, r, nq, head, QW, st, name)) return rc;
    float* PN = tab + (size_t)n_rel * n_ent * dq;
    const int evec = (d % 4 == 0 && lde % 4 == 0 && aligned16(E)) ? 1 : 0;
    const size_t lds = (size_t)(dq / 4) * PT * 16 + 4 * PT * sizeof(float);
    hipLaunchKernelGGL(rel_transr_project_kernel, dim3((unsigned)((n_ent + PT - 1) / PT), (unsigned)nr), dim3(256), lds, st, E, lde, A, lda, d,
                       dq, n_ent, evec, tab, l1 ? nullptr : PN);
    if (int rc = check_launch(name)) return rc;
    if (!l1) a.N = PN;
  }
  const int seg = topn <= TOPN_MAX ? 1 : sweep_segments(topn);
  const int rc = with_k_steps(d, [&](auto ks) {
    constexpr int KS = decltype(ks)::value;
    auto go = [&](auto sg) {
      constexpr int SEG = decltype(sg)::value;
      if (dd) return l1 ? launch_kg_topn_rel<KS, true, true, SEG>(a, st, name) : launch_kg_topn_rel<KS, false, true, SEG>(a, st, name);
      return l1 ? launch_kg_topn_rel<KS, true, false, SEG>(a, st, name) : launch_kg_topn_rel<KS, false, false, SEG>(a, st, name);
    };
    return seg == 1 ? go(std::integral_constant<int, 1>{}) : seg == 2 ? go(std::integral_constant<int, 2>{}) : go(std::integral_constant<int, 4>{});
  });
  if (rc) return rc;
  if (int e = sweep_merge<false>(a.sw, pid, psc, st, name)) return e;
  hipLaunchKernelGGL(rel_unscatter_kernel, dim3(grid_for((nq * topn + 255) / 256)), dim3(256), 0, st, key2pos, nq, topn, pid, psc, top_ids,
                     top_scores);
  return check_launch(name);
}
