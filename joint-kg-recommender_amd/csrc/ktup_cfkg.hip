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
// never writes the (users x candidates) matrix.  The sweep is ktup_sweep_pass.h's; cfkg_pass_kernel supplies the scorer: the query
// row is c = U[u] + R[rel], candidate j is entity row cand_ids[j], and
//   * squared L2: |c|^2 - 2 c.e + |e|^2 with c.e on v_mfma_f32_16x16x4_f32; |e|^2 is computed once per pass
//     (cfkg_cand_norm_kernel) and rides in the staged row's spare slot;
//   * L1: on the VALU against the same stage, the wave's 16 query rows in LDS.
// The spare slot also carries whether the candidate's entity row exists.
#include "ktup_rows.h"
#include "ktup_cfkg_norm.h"
#include "ktup_sweep_scorers.h"

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

// (the scorer, CfkgScorer, is in ktup_sweep_scorers.h and the |e|^2 launch in ktup_cfkg_norm.h: the gold-rank pass runs them too)
template <int KS, bool VEC, bool L1>
__global__ __launch_bounds__(256, 2) void cfkg_pass_kernel(CfkgPassArgs a) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  CfkgScorer<KS, L1> sc{a};
  sweep_pass<KS, VEC>(a.sw, sc, smem);
}

// the wide lists (ktup_topn.h) of ktup_eval_cfkg_topk_wide: two or four 16-key segments per user; two workgroups per CU only at the
// narrowest rows.  L1 beyond d = 192 holds 65 KB of query rows beside 65 KB of stages, which leaves 24 KB:
// the narrow lists' size.  There a stage is ONE 16-candidate tile (33 KB of stages), and the wide lists fit.
constexpr int cfkg_wide_stage(int ks, bool l1) { return l1 && ks > 48 ? 16 : 0; }

template <int KS, bool L1, int SEG>
constexpr size_t cfkg_wide_lds() {
  return SweepGeom<KS, cfkg_wide_stage(KS, L1)>::lds(CfkgScorer<KS, L1, cfkg_wide_stage(KS, L1)>::LDS, SEG);
}

template <int KS, bool VEC, bool L1, int SEG>
__global__ __launch_bounds__(256, sweep_wide_wgs(cfkg_wide_lds<KS, L1, SEG>())) void cfkg_pass_wide_kernel(CfkgPassArgs a) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  constexpr int STC = cfkg_wide_stage(KS, L1);
  CfkgScorer<KS, L1, STC> sc{a};
  sweep_pass<KS, VEC, SEG, STC>(a.sw, sc, smem);
}

template <int KS, bool L1, int SEG>
int launch_cfkg_pass(const CfkgPassArgs& a, hipStream_t st, const char* name) {
  constexpr int STC = SEG == 1 ? 0 : cfkg_wide_stage(KS, L1);
  constexpr size_t lds = SweepGeom<KS, STC>::lds(CfkgScorer<KS, L1, STC>::LDS, SEG);
  if constexpr (SEG == 1)
    return a.sw.vec ? sweep_launch<lds>(cfkg_pass_kernel<KS, true, L1>, a, a.sw, st, name) : sweep_launch<lds>(cfkg_pass_kernel<KS, false, L1>, a, a.sw, st, name);
  else
    return a.sw.vec ? sweep_launch<lds>(cfkg_pass_wide_kernel<KS, true, L1, SEG>, a, a.sw, st, name)
                    : sweep_launch<lds>(cfkg_pass_wide_kernel<KS, false, L1, SEG>, a, a.sw, st, name);
}

// both entry points; topn_max: TOPN_MAX (narrow lists) or TOPN_WIDE_MAX (wide lists, at every topn)
int cfkg_topk(const char* name, int topn_max, const float* U, int64_t ldu, const float* R, int64_t ldr, int64_t rel, const float* E, int64_t lde,
              int64_t n_ent, const int64_t* cand_ids, int64_t n_cand, int d, const int64_t* u_ids, int64_t nq, int l1,
              const int64_t* filt_off, const int32_t* filt_ids, int topn, int nsplit, int32_t* top_ids, float* top_scores, void* ws,
              void* stream) {
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
  if (topn > topn_max) return set_error(KTUP_ERR_UNSUPPORTED, "%s: topn %d > %d", name, topn, topn_max);
  if (d > 256) return set_error(KTUP_ERR_UNSUPPORTED, "%s: embedding_size %d > 256", name, d);
  if (n_cand >= ((int64_t)1 << 31)) return set_error(KTUP_ERR_UNSUPPORTED, "%s: %lld candidates do not fit 32-bit ids", name, (long long)n_cand);
  if (nq == 0) return KTUP_OK;
  hipStream_t st = (hipStream_t)stream;
  CfkgPassArgs a;
  a.U = U; a.ldu = ldu; a.R = R; a.ldr = ldr; a.rel = rel; a.E = E; a.lde = lde; a.n_ent = n_ent; a.cand_ids = cand_ids; a.enorm = nullptr;
  a.sw.u_ids = u_ids; a.sw.nq = nq; a.sw.n = n_cand; a.sw.d = d; a.sw.topn = topn;
  a.sw.vec = (d % 4 == 0 && lde % 4 == 0 && (reinterpret_cast<uintptr_t>(E) & 15) == 0) ? 1 : 0;
  float* en = nullptr;
  if (int rc = sweep_prepare(a.sw, nsplit, filt_off, filt_ids, ws, &en, st, name)) return rc;
  if (!l1) {
    hipLaunchKernelGGL(cfkg_cand_norm_kernel, dim3((unsigned)min((n_cand + 15) / 16, (int64_t)4096)), dim3(256), 0, st, E, lde, n_ent, cand_ids,
                       n_cand, d, en);
    if (int rc = check_launch(name)) return rc;
    a.enorm = en;
  }
  const int seg = topn_max == TOPN_MAX ? 1 : sweep_segments(topn);
  const int rc = with_k_steps(d, [&](auto ks) {
    constexpr int KS = decltype(ks)::value;
    auto go = [&](auto sg) {
      constexpr int SEG = decltype(sg)::value;
      return l1 ? launch_cfkg_pass<KS, true, SEG>(a, st, name) : launch_cfkg_pass<KS, false, SEG>(a, st, name);
    };
    return seg == 1 ? go(std::integral_constant<int, 1>{}) : seg == 2 ? go(std::integral_constant<int, 2>{}) : go(std::integral_constant<int, 4>{});
  });
  return rc ? rc : sweep_merge<false>(a.sw, top_ids, top_scores, st, name);
}

}  // namespace
}  // namespace ktup

extern "C" size_t ktup_eval_cfkg_topk_workspace_bytes(int d, int64_t nq, int64_t n_cand, int topn, int nsplit) {
  (void)d;
  return sweep_workspace_bytes(nq, n_cand, topn, TOPN_MAX, nsplit, 1);
}

extern "C" int ktup_eval_cfkg_topk(const float* U, int64_t ldu, const float* R, int64_t ldr, int64_t rel, const float* E, int64_t lde,
                                   int64_t n_ent, const int64_t* cand_ids, int64_t n_cand, int d, const int64_t* u_ids, int64_t nq, int l1,
                                   const int64_t* filt_off, const int32_t* filt_ids, int topn, int nsplit, int32_t* top_ids,
                                   float* top_scores, void* ws, void* stream) {
  return cfkg_topk("ktup_eval_cfkg_topk", TOPN_MAX, U, ldu, R, ldr, rel, E, lde, n_ent, cand_ids, n_cand, d, u_ids, nq, l1, filt_off, filt_ids,
                   topn, nsplit, top_ids, top_scores, ws, stream);
}

extern "C" size_t ktup_eval_cfkg_topk_wide_workspace_bytes(int d, int64_t nq, int64_t n_cand, int topn, int nsplit) {
  (void)d;
  return sweep_workspace_bytes(nq, n_cand, topn, TOPN_WIDE_MAX, nsplit, 1);
}

extern "C" int ktup_eval_cfkg_topk_wide(const float* U, int64_t ldu, const float* R, int64_t ldr, int64_t rel, const float* E, int64_t lde,
                                        int64_t n_ent, const int64_t* cand_ids, int64_t n_cand, int d, const int64_t* u_ids, int64_t nq,
                                        int l1, const int64_t* filt_off, const int32_t* filt_ids, int topn, int nsplit, int32_t* top_ids,
                                        float* top_scores, void* ws, void* stream) {
  return cfkg_topk("ktup_eval_cfkg_topk_wide", TOPN_WIDE_MAX, U, ldu, R, ldr, rel, E, lde, n_ent, cand_ids, n_cand, d, u_ids, nq, l1, filt_off,
                   filt_ids, topn, nsplit, top_ids, top_scores, ws, stream);
}
