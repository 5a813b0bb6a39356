// Link prediction as lists: the filtered top-n ENTITIES of every key (q, r) in one sweep that never writes the (keys x candidates)
// matrix -- "which tails complete (h, r, ?)" / "which heads complete (?, r, t)" with the scores of evaluateHead / evaluateTail
// (transE.py:65-105, transH.py:73-121).  See include/ktup_hip.h, ktup_eval_kg_topk.
//
// The sweep is ktup_sweep_pass.h's (64 keys per workgroup, candidate rows through a double-buffered LDS stage, filter bits, the sorted
// 16-key list segments of ktup_topn.h, the split merge); this file supplies the scorer.  Its query is a KEY, not a table row:
// kg_query_prep (ktup_eval.hip) writes c -- E[q] + R[r] (tail) or E[q] - R[r] (head), for TransH with E[q] projected onto the
// relation's hyperplane first -- and TransH's normal w = Nrm[r] for all keys into the workspace, kg_topn_keys_kernel adds the iota the
// sweep indexes them by and TransH's scalars w.c and |w|^2, and the scorer's query(u, k) reads row u of that.  Per key and candidate e:
//   * TransE, squared L2:  |c|^2 - 2 c.e + |e|^2, c.e on v_mfma_f32_16x16x4_f32 (the arithmetic of CfkgScorer, ktup_cfkg.hip);
//   * TransH, squared L2:  |c|^2 - 2 c.e + |e|^2 + (w.e) (2 w.c - (2 - |w|^2) (w.e))  (|w| = 1 is NOT assumed): w.e is a second MFMA
//     chain against the same staged tile, the key's w row held as a second register operand; the w.e term is folded into the
//     accumulator before the sweep ranks it;
//   * L1 (VALU, against the same stage; a wave's 16 c rows in LDS): TransE sum |c_k - e_k|; TransH first w.e (on the matrix cores,
//     from the register operand), then sum |c_k - e_k + (w.e) w_k|.  c and w rows of 64 keys would be 133 KB of LDS at d = 256, so
//     TransH keeps both as register operands and passes them through 8.5 KB of LDS a wave, 16 k quads at a time, once per stage.
// |e|^2 is computed once per pass (kg_topn_cand_norm_kernel) and rides in the staged row's spare slot.  A score is a function of the
// (key, candidate) pair's own chains only: the same bits at every list width, stage size and split count.
#include "ktup_pref_geom.h"
#include "ktup_sweep_pass.h"

using namespace ktup;

namespace ktup {
namespace {

// per key: its position (the sweep's u_ids) and, for TransH, {w.c, |w|^2} from kg_query_prep's rows.  16 lanes per key.
__global__ __launch_bounds__(256) void kg_topn_keys_kernel(const float* __restrict__ QW, int dq, int64_t nq, int transh,
                                                           int64_t* __restrict__ iota, float* __restrict__ QS) {
  const int l = threadIdx.x & 15;
  for (int64_t b = (int64_t)blockIdx.x * 16 + (threadIdx.x >> 4); b < nq; b += (int64_t)gridDim.x * 16) {
    if (l == 0) iota[b] = b;
    if (!transh) continue;
    const float* c = QW + b * 3 * dq;
    const float* w = c + 2 * dq;
    float wc = 0.f, ww = 0.f;
    for (int k = l; k < dq; k += 16) {                                     // (the rows are zero past the width)
      wc = fmaf(w[k], c[k], wc);
      ww = fmaf(w[k], w[k], ww);
    }
    wc = group_sum<16>(wc);
    ww = group_sum<16>(ww);
    if (l == 0) { QS[2 * b] = wc; QS[2 * b + 1] = ww; }
  }
}

// |e|^2 of every candidate row, once per pass (squared L2 only): 16 lanes per candidate (cfkg_cand_norm_kernel without the gather)
__global__ __launch_bounds__(256) void kg_topn_cand_norm_kernel(const float* __restrict__ C, int64_t ldc, int64_t n_cand, int d,
                                                                float* __restrict__ out) {
  const int l = threadIdx.x & 15;
  for (int64_t c = (int64_t)blockIdx.x * 16 + (threadIdx.x >> 4); c < n_cand; c += (int64_t)gridDim.x * 16) {
    const float* row = C + c * ldc;
    float s = 0.f;
    for (int k = l; k < d; k += 16) s = fmaf(row[k], row[k], s);
    s = group_sum<16>(s);
    if (l == 0) out[c] = s;
  }
}

struct KgTopnArgs {
  SweepArgs sw;
  const float* QW; int dq;              // [nq][3][dq]: slot 0 = c, slot 2 = w (TransH)
  const float* QS;                      // [nq][2]: w.c, |w|^2 (TransH)
  const float* C; int64_t ldc;          // the candidate rows
  const float* enorm;                   // [n_cand] |e|^2 (squared L2); NULL under L1
};

// NSUB dot products of a stage on v_mfma_f32_16x16x4_f32, k ascending (sweep_tile_dot for any stage size)
template <int KS, int NSUB>
KTUP_DEV void kg_tile_dot(const float (&av)[KS], const v4* eb, int kq, v4 (&acc)[NSUB]) {
  constexpr int ROW4 = SweepGeom<KS>::ROW4;
  const float* rb = reinterpret_cast<const float*>(eb) + kq;               // lane (kq, candidate j): element kq of every k quad
#pragma unroll
  for (int s = 0; s < KS; ++s) {
#pragma unroll
    for (int t = 0; t < NSUB; ++t) acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[s], rb[t * 16 * ROW4 * 4 + 4 * s], acc[t], 0, 0, 0);
  }
}

// What kg_topn_kernel adds to the sweep.  The sweep ranks s = -distance descending: ascending distance, ties -> lower candidate.
// H: TransH.
template <int KS, bool L1, bool H, int STC = 0>
struct KgScorer {
  using G = SweepGeom<KS, STC>;
  // L1, TransE: a wave's 16 c rows in LDS for the whole pass, [16][CROW4] float4 (CfkgScorer's).  L1, TransH: c AND w rows would be
  // 133 KB at d = 256, so the wave keeps both as register operands and hands them to its LDS KC k quads at a time, once per stage:
  // [2][16][CHP] float4, 8.5 KB a wave at every width (128 ds_write_b32 a lane and stage at d = 256, beside ~6,000 VALU operations).
  static constexpr int CROW4 = KS | 1;
  static constexpr int KC = 16, CHP = KC | 1;
  static constexpr size_t CW = !L1 ? 0 : H ? (size_t)2 * 16 * CHP * 16 : (size_t)16 * CROW4 * 16;
  static constexpr size_t LDS = 4 * CW;
  const KgTopnArgs& a;
  float cn[4] = {0.f, 0.f, 0.f, 0.f};                                     // squared L2: |c|^2 of the keys of this lane's accumulator rows
  float wc2[4] = {0.f, 0.f, 0.f, 0.f};                                    // TransH, squared L2: 2 w.c of those keys
  float k2[4] = {0.f, 0.f, 0.f, 0.f};                                     //   ... and 2 - |w|^2
  const v4* cw = nullptr;                                                 // L1: the c rows of those four keys, [4][CROW4] (TransH: [4][CHP])
  float* put = nullptr;                                                   // L1, TransH: where this lane's operands go, key j's row, element kq
  float wv[H ? KS : 1];                                                   // TransH: the A operand of w.e -- element 4 s + kq of key j's w row
  KTUP_DEV float query(int64_t u, int k) const { return a.QW[u * 3 * a.dq + k]; }
  KTUP_DEV void hold(const float (&av)[KS], char* smem, int64_t u0, const bool (&in)[4], int kq, int j) {
    if constexpr (H) {
      const bool ok = u0 + j < a.sw.nq;
      const float* w = a.QW + ((ok ? u0 + j : (int64_t)0) * 3 + 2) * a.dq;
#pragma unroll
      for (int s = 0; s < KS; ++s) wv[s] = w[min(4 * s + kq, a.sw.d - 1)];
#pragma unroll
      for (int s = 0; s < KS; ++s) wv[s] = (ok && 4 * s + kq < a.sw.d) ? wv[s] : 0.f;
    }
    if constexpr (L1 && H) {
      float* cwf = reinterpret_cast<float*>(smem + (size_t)__builtin_amdgcn_readfirstlane(threadIdx.x >> 6) * CW);   // [2][16][CHP] float4
      put = cwf + j * CHP * 4 + kq;
      cw = reinterpret_cast<const v4*>(cwf) + 4 * kq * CHP;
    } else if constexpr (L1) {
      float* cwf = reinterpret_cast<float*>(smem + (size_t)__builtin_amdgcn_readfirstlane(threadIdx.x >> 6) * CW);   // [16][CROW4] float4
#pragma unroll
      for (int s = 0; s < KS; ++s) cwf[(j * CROW4 + s) * 4 + kq] = av[s];
      cw = reinterpret_cast<const v4*>(cwf) + 4 * kq * CROW4;
    } else {
      float cnj = 0.f;
#pragma unroll
      for (int s = 0; s < KS; ++s) cnj = fmaf(av[s], av[s], cnj);
      cnj += __shfl_xor(cnj, 16, 64);
      cnj += __shfl_xor(cnj, 32, 64);                                     // |c|^2 of key j on every lane (., j)
#pragma unroll
      for (int reg = 0; reg < 4; ++reg) cn[reg] = __shfl(cnj, 4 * kq + reg, 64);
      if constexpr (H) {
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) {
          const int64_t p = in[reg] ? u0 + 4 * kq + reg : (int64_t)0;
          const float wc = a.QS[2 * p], ww = a.QS[2 * p + 1];
          wc2[reg] = in[reg] ? 2.f * wc : 0.f;
          k2[reg] = in[reg] ? 2.f - ww : 0.f;
        }
      }
    }
  }
  KTUP_DEV const float* row(int64_t c, bool& live) const {
    live = true;
    return a.C + c * a.ldc;
  }
  KTUP_DEV v4 spare(int64_t c, bool) const { return (v4){a.enorm ? a.enorm[c] : 0.f, 1.f, 0.f, 0.f}; }
  // acc[t][reg] of key 4 kq + reg x candidate 16 t + j.  Squared L2: c.e, for TransH less (w.e) (2 w.c - (2 - |w|^2) (w.e)) / 2, so that
  // score() is TransE's expression for both.  L1: the distance itself.
  KTUP_DEV void tile_math(const float (&av)[KS], const v4* eb, int kq, v4 (&acc)[G::NSUB]) const {
    v4 we[G::NSUB];
    if constexpr (H) {
#pragma unroll
      for (int t = 0; t < G::NSUB; ++t) we[t] = (v4){0.f, 0.f, 0.f, 0.f};
      kg_tile_dot<KS, G::NSUB>(wv, eb, kq, we);
    }
    if constexpr (L1 && H) {
      // KC k quads at a time: every lane stores its operands of the chunk (static register indices: the chunk loop is unrolled), the
      // wave reads them back as rows.  LDS operations of one wave complete in order; the fences keep the compiler from moving them.
#pragma unroll
      for (int c0 = 0; c0 < KS; c0 += KC) {
        const int n = KS - c0 < KC ? KS - c0 : KC;
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
#pragma unroll
        for (int sl = 0; sl < KC; ++sl) {
          if (c0 + sl < KS) {
            put[sl * 4] = av[c0 + sl];
            put[(16 * CHP + sl) * 4] = wv[c0 + sl];
          }
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
#pragma unroll 2
        for (int sl = 0; sl < n; ++sl) {
          v4 cq[4], wq[4];
#pragma unroll
          for (int reg = 0; reg < 4; ++reg) {
            cq[reg] = cw[reg * CHP + sl];
            wq[reg] = cw[(16 + reg) * CHP + sl];
          }
#pragma unroll
          for (int t = 0; t < G::NSUB; ++t) {
            const v4 e = eb[t * 16 * G::ROW4 + c0 + sl];
#pragma unroll
            for (int reg = 0; reg < 4; ++reg) {
              v4 z = cq[reg] - e;
#pragma unroll
              for (int q = 0; q < 4; ++q) z[q] = fmaf(we[t][reg], wq[reg][q], z[q]);
              acc[t][reg] += (fabsf(z[0]) + fabsf(z[1])) + (fabsf(z[2]) + fabsf(z[3]));
            }
          }
        }
      }
    } else if constexpr (L1) {
#pragma unroll 2
      for (int s = 0; s < KS; ++s) {
        v4 cq[4];
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) cq[reg] = cw[reg * CROW4 + s];
#pragma unroll
        for (int t = 0; t < G::NSUB; ++t) {
          const v4 e = eb[t * 16 * G::ROW4 + s];
#pragma unroll
          for (int reg = 0; reg < 4; ++reg) {
            const v4 z = cq[reg] - e;
            acc[t][reg] += (fabsf(z[0]) + fabsf(z[1])) + (fabsf(z[2]) + fabsf(z[3]));
          }
        }
      }
    } else {
      kg_tile_dot<KS, G::NSUB>(av, eb, kq, acc);
      if constexpr (H) {
#pragma unroll
        for (int t = 0; t < G::NSUB; ++t) {
#pragma unroll
          for (int reg = 0; reg < 4; ++reg) {
            const float x = we[t][reg];
            acc[t][reg] = fmaf(-0.5f * x, fmaf(-k2[reg], x, wc2[reg]), acc[t][reg]);
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

// TransE with L1 beyond d = 192 holds 65 KB of c rows beside 65 KB of stages, which leaves room for the narrow lists only: under the
// wide lists a stage is ONE 16-candidate tile there (cfkg_wide_stage's rule)
// TransH with squared L2 holds TWO register operands (c and w rows: 2 KS registers a lane).  Where two workgroups per CU fit the LDS
// they leave 256 registers each: at d = 36 - 100 (KS = 16, 25) that holds without scratch once the stage is halved to 32 candidates
// (two accumulators per chain instead of four, half the loads in flight); from d = 101 on (KS >= 32) the kernel is compiled for ONE
// workgroup per CU and 512 registers.
constexpr int kg_topn_stage(int ks, bool l1, bool h, int seg) {
  return seg > 1 && l1 && !h && ks > 48 ? 16 : h && !l1 && (ks == 16 || ks == 25) ? 32 : 0;
}

template <int KS, bool L1, bool H, int SEG>
constexpr size_t kg_topn_lds() {
  constexpr int STC = kg_topn_stage(KS, L1, H, SEG);
  return SweepGeom<KS, STC>::lds(KgScorer<KS, L1, H, STC>::LDS, SEG);
}

// registers bounded for the workgroups per CU the LDS admits (sweep_wide_wgs): one workgroup and 512 registers a lane at the wide rows
template <int KS, bool L1, bool H, int SEG>
constexpr int kg_topn_wgs() { return H && !L1 && KS >= 32 ? 1 : sweep_wide_wgs(kg_topn_lds<KS, L1, H, SEG>()); }

template <int KS, bool VEC, bool L1, bool H, int SEG>
__global__ __launch_bounds__(256, (kg_topn_wgs<KS, L1, H, SEG>())) void kg_topn_kernel(KgTopnArgs a) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  constexpr int STC = kg_topn_stage(KS, L1, H, SEG);
  KgScorer<KS, L1, H, STC> sc{a};
  sweep_pass<KS, VEC, SEG, STC>(a.sw, sc, smem);
}

template <int KS, bool L1, bool H, int SEG>
int launch_kg_topn(const KgTopnArgs& a, hipStream_t st, const char* name) {
  constexpr size_t lds = kg_topn_lds<KS, L1, H, SEG>();
  return a.sw.vec ? sweep_launch<lds>(kg_topn_kernel<KS, true, L1, H, SEG>, a, a.sw, st, name)
                  : sweep_launch<lds>(kg_topn_kernel<KS, false, L1, H, SEG>, a, a.sw, st, name);
}

inline int round4(int d) { return (d + 3) / 4 * 4; }
inline size_t up16(size_t x) { return (x + 15) & ~(size_t)15; }
inline bool kg_topn_covers(int model, int d, int topn) {
  return (model == KTUP_KG_TRANSE || model == KTUP_KG_TRANSH) && d >= 1 && d <= 256 && topn >= 1 && topn <= TOPN_WIDE_MAX;
}

}  // namespace
}  // namespace ktup

extern "C" int ktup_eval_kg_topk_supported(int model, int d, int l1, int topn) {
  (void)l1;
  return kg_topn_covers(model, d, topn) ? 1 : 0;
}

// the sweep's workspace (partial lists | filter bits | |e|^2) | key positions [nq] int64 | QW [nq][3][round4(d)] | QS [nq][2]
extern "C" size_t ktup_eval_kg_topk_workspace_bytes(int model, int d, int64_t nq, int64_t n_cand, int64_t n_rel, int topn, int nsplit) {
  (void)n_rel;
  if (!kg_topn_covers(model, d, topn) || n_cand >= ((int64_t)1 << 31)) return 0;
  const size_t sweep = sweep_workspace_bytes(nq, n_cand, topn, TOPN_WIDE_MAX, nsplit, 1);
  if (!sweep) return 0;
  return up16(sweep) + up16((size_t)nq * sizeof(int64_t)) + up16((size_t)nq * 3 * round4(d) * sizeof(float)) +
         up16((size_t)nq * 2 * sizeof(float)) + 16;
}

extern "C" int ktup_eval_kg_topk(int model, const float* E, int64_t lde, const float* R, int64_t ldr, const float* Nrm, int64_t ldn,
                                 int64_t n_rel, int d, const float* C, int64_t ldc, int64_t n_cand, const int64_t* q, const int64_t* r,
                                 int64_t nq, int l1, int head, const int64_t* filt_off, const int32_t* filt_ids, int topn, int nsplit,
                                 int32_t* top_ids, float* top_scores, void* ws, void* stream) {
  const char* name = "ktup_eval_kg_topk";
  if (model != KTUP_KG_TRANSE && model != KTUP_KG_TRANSH)
    return set_error(KTUP_ERR_UNSUPPORTED, "%s: model %d is neither KTUP_KG_TRANSE nor KTUP_KG_TRANSH", name, model);
  const bool transh = model == KTUP_KG_TRANSH;
  KTUP_REQUIRE(E, "%s: null entity table E", name);
  KTUP_REQUIRE(R, "%s: null relation table R", name);
  KTUP_REQUIRE(!transh || Nrm, "%s: null norm table Nrm (KTUP_KG_TRANSH)", name);
  KTUP_REQUIRE(C, "%s: null candidate table C", name);
  KTUP_REQUIRE(q && r, "%s: null key ids (q, r)", name);
  KTUP_REQUIRE(top_ids, "%s: null output top_ids", name);
  KTUP_REQUIRE(ws, "%s: null workspace ws", name);
  KTUP_REQUIRE(d >= 1 && nq >= 0 && n_cand > 0 && n_rel > 0 && topn > 0 && nsplit >= 0,
               "%s: bad sizes (embedding_size d %d, nq %lld, n_cand %lld, n_rel %lld, topn %d, nsplit %d)", name, d, (long long)nq,
               (long long)n_cand, (long long)n_rel, topn, nsplit);
  KTUP_REQUIRE(lde >= d && ldr >= d && ldc >= d && (!transh || ldn >= d), "%s: a row pitch (lde, ldr, ldn, ldc) is below embedding_size %d",
               name, d);
  KTUP_REQUIRE((filt_off == nullptr) == (filt_ids == nullptr), "%s: filt_off and filt_ids go together", name);
  KTUP_REQUIRE((reinterpret_cast<uintptr_t>(ws) & 15) == 0, "%s: the workspace ws must be 16-byte aligned", name);
  if (topn > TOPN_WIDE_MAX) return set_error(KTUP_ERR_UNSUPPORTED, "%s: topn %d > %d", name, topn, TOPN_WIDE_MAX);
  if (d > 256) return set_error(KTUP_ERR_UNSUPPORTED, "%s: embedding_size %d > 256", name, d);
  if (n_cand >= ((int64_t)1 << 31)) return set_error(KTUP_ERR_UNSUPPORTED, "%s: n_cand %lld does not fit 32-bit ids", name, (long long)n_cand);
  if (nq == 0) return KTUP_OK;
  hipStream_t st = (hipStream_t)stream;
  const int dq = round4(d);
  char* extra = reinterpret_cast<char*>(ws) + up16(sweep_workspace_bytes(nq, n_cand, topn, TOPN_WIDE_MAX, nsplit, 1));
  int64_t* iota = reinterpret_cast<int64_t*>(extra);
  float* QW = reinterpret_cast<float*>(extra + up16((size_t)nq * sizeof(int64_t)));
  float* QS = QW + up16((size_t)nq * 3 * dq * sizeof(float)) / sizeof(float);
  KgTopnArgs a;
  a.QW = QW; a.dq = dq; a.QS = QS; a.C = C; a.ldc = ldc; a.enorm = nullptr;
  a.sw.u_ids = iota; a.sw.nq = nq; a.sw.n = n_cand; a.sw.d = d; a.sw.topn = topn;
  a.sw.vec = (d % 4 == 0 && ldc % 4 == 0 && aligned16(C)) ? 1 : 0;
  float* en = nullptr;
  if (int rc = sweep_prepare(a.sw, nsplit, filt_off, filt_ids, ws, &en, st, name)) return rc;
  if (int rc = kg_query_prep(model, E, lde, R, ldr, Nrm, ldn, d, q, r, nq, head, QW, st, name)) return rc;
  hipLaunchKernelGGL(kg_topn_keys_kernel, dim3(grid_for((nq + 15) / 16)), dim3(256), 0, st, QW, dq, nq, transh ? 1 : 0, iota, QS);
  if (int rc = check_launch(name)) return rc;
  if (!l1) {
    hipLaunchKernelGGL(kg_topn_cand_norm_kernel, dim3((unsigned)min((n_cand + 15) / 16, (int64_t)4096)), dim3(256), 0, st, C, ldc, n_cand, d, en);
    if (int rc = check_launch(name)) return rc;
    a.enorm = en;
  }
  const int seg = topn <= TOPN_MAX ? 1 : sweep_segments(topn);
  const int rc = with_k_steps(d, [&](auto ks) {
    constexpr int KS = decltype(ks)::value;
    auto go = [&](auto sg) {
      constexpr int SEG = decltype(sg)::value;
      if (transh) return l1 ? launch_kg_topn<KS, true, true, SEG>(a, st, name) : launch_kg_topn<KS, false, true, SEG>(a, st, name);
      return l1 ? launch_kg_topn<KS, true, false, SEG>(a, st, name) : launch_kg_topn<KS, false, false, SEG>(a, st, name);
    };
    return seg == 1 ? go(std::integral_constant<int, 1>{}) : seg == 2 ? go(std::integral_constant<int, 2>{}) : go(std::integral_constant<int, 4>{});
  });
  return rc ? rc : sweep_merge<false>(a.sw, top_ids, top_scores, st, name);
}
