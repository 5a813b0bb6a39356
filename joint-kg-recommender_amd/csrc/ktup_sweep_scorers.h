// The two rec SCORERS of the one-sweep passes (ktup_sweep_pass.h says what a scorer supplies), in a header because two kinds of pass
// run them: the top-n list passes (ktup_dot_pass.hip, ktup_cfkg.hip) and the gold-rank passes (ktup_rank_pass.hip), whose ranks
// are counts against the very keys the list passes order by -- one copy of tile_math / score / live, hence one set of score bits.
//   DotScorer   the inner-product recommenders (BPRMF, FM, CKE, coFM): query row U[u], candidate j = item row j, the item's additive
//               term in the row's spare slot; a score is the MFMA dot product -- bit for bit the fmaf chain of K11 (bprmf_eval_kernel)
//               -- then the two separately rounded adds.
//   CfkgScorer  CFKG: query row c = U[u] + R[rel], candidate j = entity row cand_ids[j]; squared L2 as |c|^2 - 2 c.e + |e|^2 with c.e
//               on v_mfma_f32_16x16x4_f32 (|e|^2 once per pass by cfkg_cand_norm_kernel, ktup_cfkg_norm.h, in the spare slot), L1 on
//               the VALU against the same stage with the wave's 16 query rows in LDS.  The spare slot also says whether the candidate
//               has a row.
#pragma once
#include "ktup_sweep_pass.h"

namespace ktup {
namespace {

struct DotArgs {
  const float* U; int64_t ldu;
  const float* I; int64_t ldi;
  const float *user_add, *item_add;     // NULL = none
  SweepArgs sw;
};

template <int KS>
struct DotScorer {
  static constexpr size_t LDS = 0;
  const DotArgs& a;
  float uadd[4] = {0.f, 0.f, 0.f, 0.f};
  KTUP_DEV float query(int64_t u, int k) const { return a.U[u * a.ldu + k]; }
  KTUP_DEV void hold(const float (&)[KS], char*, int64_t u0, const bool (&in)[4], int kq, int) {
#pragma unroll
    for (int reg = 0; reg < 4; ++reg)
      if (a.user_add && in[reg]) uadd[reg] = a.user_add[u0 + 4 * kq + reg];
  }
  KTUP_DEV const float* row(int64_t c, bool& live) const { live = true; return a.I + c * a.ldi; }
  KTUP_DEV v4 spare(int64_t c, bool) const { return (v4){a.item_add ? a.item_add[c] : 0.f, 0.f, 0.f, 0.f}; }
  KTUP_DEV void tile_math(const float (&av)[KS], const v4* eb, int kq, v4 (&acc)[SweepGeom<KS>::NSUB]) const { sweep_tile_dot<KS>(av, eb, kq, acc); }
  KTUP_DEV float staged(const v4* slot) const { return *reinterpret_cast<const float*>(slot); }
  KTUP_DEV bool live(float) const { return true; }
  KTUP_DEV float score(float dot, int reg, float iadd) const {
    float s = dot;
    if (a.user_add) s = __fadd_rn(s, uadd[reg]);
    if (a.item_add) s = __fadd_rn(s, iadd);
    return s;
  }
};

struct CfkgPassArgs {
  SweepArgs sw;
  const float* U; int64_t ldu;
  const float* R; int64_t ldr, rel;
  const float* E; int64_t lde, n_ent;
  const int64_t* cand_ids;              // NULL: candidate j is row j
  const float* enorm;                   // [n_cand] |e|^2 (squared L2); NULL under L1
};

// What cfkg_pass_kernel adds to the sweep.  The sweep ranks s = -distance descending, like the inner-product pass: ascending
// distance, ties -> lower j.
template <int KS, bool L1, int STC = 0>
struct CfkgScorer {
  using G = SweepGeom<KS, STC>;
  static constexpr int CROW4 = KS | 1;                                    // L1: float4 pitch of a query row in LDS
  static constexpr size_t CW = L1 ? (size_t)16 * CROW4 * 16 : 0;          // L1: a wave's 16 query rows
  static constexpr size_t LDS = 4 * CW;
  const CfkgPassArgs& a;
  float cn[4] = {0.f, 0.f, 0.f, 0.f};                                     // squared L2: |c|^2 of the users of this lane's accumulator rows
  const v4* cw = nullptr;                                                 // L1: the query rows of those four users, [4][CROW4]
  KTUP_DEV float query(int64_t u, int k) const { return a.U[u * a.ldu + k] + a.R[a.rel * a.ldr + k]; }
  KTUP_DEV void hold(const float (&av)[KS], char* smem, int64_t, const bool (&)[4], int kq, int j) {
    if constexpr (L1) {
      float* cwf = reinterpret_cast<float*>(smem + (size_t)__builtin_amdgcn_readfirstlane(threadIdx.x >> 6) * CW);   // [16][CROW4] float4
#pragma unroll
      for (int s = 0; s < KS; ++s) cwf[(j * CROW4 + s) * 4 + kq] = av[s];
      cw = reinterpret_cast<const v4*>(cwf) + 4 * kq * CROW4;
    } else {
      float cnj = 0.f;
#pragma unroll
      for (int s = 0; s < KS; ++s) cnj = fmaf(av[s], av[s], cnj);
      cnj += __shfl_xor(cnj, 16, 64);
      cnj += __shfl_xor(cnj, 32, 64);                                     // |c|^2 of user j on every lane (., j)
#pragma unroll
      for (int reg = 0; reg < 4; ++reg) cn[reg] = __shfl(cnj, 4 * kq + reg, 64);
    }
  }
  // a cand_ids entry outside [0, n_ent) is never ranked and never dereferenced: the stage reads row 0 in its place
  KTUP_DEV const float* row(int64_t c, bool& live) const {
    const int64_t id = a.cand_ids ? a.cand_ids[c] : c;
    live = id >= 0 && id < a.n_ent;
    return a.E + (live ? id : (int64_t)0) * a.lde;
  }
  KTUP_DEV v4 spare(int64_t c, bool live) const { return (v4){a.enorm ? a.enorm[c] : 0.f, live ? 1.f : 0.f, 0.f, 0.f}; }
  // acc: c.e on the matrix cores (squared L2), or the distance itself on the VALU against the same stage (L1): every lane owns the
  // 4 users x 16-candidate-tile slots the MFMA would have given it
  KTUP_DEV void tile_math(const float (&av)[KS], const v4* eb, int kq, v4 (&acc)[G::NSUB]) const {
    if constexpr (L1) {
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
      sweep_tile_dot<KS>(av, eb, kq, acc);
    }
  }
  KTUP_DEV v4 staged(const v4* slot) const { return *slot; }
  KTUP_DEV bool live(const v4& spare) const { return spare[1] != 0.f; }
  KTUP_DEV float score(float acc, int reg, const v4& spare) const {
    return -(L1 ? acc : __fadd_rn(fmaf(-2.f, acc, cn[reg]), spare[0]));    // |c|^2 - 2 c.e + |e|^2
  }
};

}  // namespace
}  // namespace ktup
