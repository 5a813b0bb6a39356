// K11 + K17 fused for a whole evaluation pass of the inner-product recommenders (BPRMF, FM, CKE, coFM): all-item scores
//     score(b, j) = (U[u_b] . I[j] + user_add[b]) + item_add[j]
// AND the filtered top-n of every user in ONE sweep that never writes the (users x items) score matrix.
//
// Reference: bprmf.py:51-54 / fm.py:69-80 / CKE.py:142-153 / cofm.py:127-141 produce a (B x N) matrix per batch of 512 users,
// which utils/misc.py:186-248 copies to the host, argsorts and walks.  The per-batch route of this build keeps that shape on the
// device (ktup_eval_bprmf_scores, two torch adds, ktup_eval_topk_filtered, ktup_eval_rec_metrics per batch).  Here the sweep is
// ktup_sweep_pass.h's; dot_pass_kernel supplies the scorer (DotScorer, ktup_sweep_scorers.h: the gold-rank pass runs it too): the query row is U[u], candidate j is item row j, the item's additive
// term rides in the row's spare slot, and a score is the MFMA dot product -- bit for bit the fmaf chain of K11 (bprmf_eval_kernel)
// -- then the two separately rounded adds, so the scores and with them the ranked lists are the per-batch route's bits.
// ktup_eval_dot_topk keeps a user's list as one key per lane (topn <= 16); ktup_eval_dot_topk_wide is the same pass on lists of two
// or four 16-key segments (dot_pass_wide_kernel: topn <= 32, <= 64).
#include "ktup_sweep_scorers.h"

namespace ktup {
namespace {

template <int KS, bool VEC>
__global__ __launch_bounds__(256, 2) void dot_pass_kernel(DotArgs a) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  DotScorer<KS> sc{a};
  sweep_pass<KS, VEC>(a.sw, sc, smem);
}

// the wide lists: two workgroups per CU up to d = 64 with two segments, one otherwise
template <int KS, bool VEC, int SEG>
__global__ __launch_bounds__(256, sweep_wide_wgs(SweepGeom<KS>::lds(DotScorer<KS>::LDS, SEG))) void dot_pass_wide_kernel(DotArgs a) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  DotScorer<KS> sc{a};
  sweep_pass<KS, VEC, SEG>(a.sw, sc, smem);
}

template <int KS, int SEG>
int launch_dot_pass(const DotArgs& a, hipStream_t st, const char* name) {
  constexpr size_t lds = SweepGeom<KS>::lds(DotScorer<KS>::LDS, SEG);
  if constexpr (SEG == 1)
    return a.sw.vec ? sweep_launch<lds>(dot_pass_kernel<KS, true>, a, a.sw, st, name) : sweep_launch<lds>(dot_pass_kernel<KS, false>, a, a.sw, st, name);
  else
    return a.sw.vec ? sweep_launch<lds>(dot_pass_wide_kernel<KS, true, SEG>, a, a.sw, st, name)
                    : sweep_launch<lds>(dot_pass_wide_kernel<KS, false, SEG>, a, a.sw, st, name);
}

// both entry points; topn_max: TOPN_MAX (narrow lists) or TOPN_WIDE_MAX (wide lists, at every topn)
int dot_topk(const char* name, int topn_max, const float* U, int64_t ldu, const float* I, int64_t ldi, int d, const int64_t* u_ids, int64_t nq,
             int64_t n_items, const float* user_add, const float* item_add, const int64_t* filt_off, const int32_t* filt_ids, int topn,
             int nsplit, int32_t* top_ids, float* top_scores, void* ws, void* stream) {
  KTUP_REQUIRE(U && I && u_ids && top_ids && ws, "%s: null table, id, output or workspace pointer", name);
  KTUP_REQUIRE(d >= 1 && nq >= 0 && n_items > 0 && topn > 0 && nsplit >= 0, "%s: bad sizes (embedding_size %d, %lld users, %lld items, topn %d, nsplit %d)",
               name, d, (long long)nq, (long long)n_items, topn, nsplit);
  KTUP_REQUIRE(ldu >= d && ldi >= d, "%s: a row pitch is below embedding_size %d", name, d);
  KTUP_REQUIRE((filt_off == nullptr) == (filt_ids == nullptr), "%s: filt_off and filt_ids go together", name);
  KTUP_REQUIRE((reinterpret_cast<uintptr_t>(ws) & 15) == 0, "%s: the workspace must be 16-byte aligned", name);
  if (topn > topn_max) return set_error(KTUP_ERR_UNSUPPORTED, "%s: topn %d > %d", name, topn, topn_max);
  if (d > 256) return set_error(KTUP_ERR_UNSUPPORTED, "%s: embedding_size %d > 256", name, d);
  if (n_items >= ((int64_t)1 << 31)) return set_error(KTUP_ERR_UNSUPPORTED, "%s: %lld items do not fit 32-bit ids", name, (long long)n_items);
  if (nq == 0) return KTUP_OK;
  hipStream_t st = (hipStream_t)stream;
  DotArgs a;
  a.U = U; a.ldu = ldu; a.I = I; a.ldi = ldi; a.user_add = user_add; a.item_add = item_add;
  a.sw.u_ids = u_ids; a.sw.nq = nq; a.sw.n = n_items; a.sw.d = d; a.sw.topn = topn;
  a.sw.vec = (d % 4 == 0 && ldi % 4 == 0 && (reinterpret_cast<uintptr_t>(I) & 15) == 0) ? 1 : 0;
  if (int rc = sweep_prepare(a.sw, nsplit, filt_off, filt_ids, ws, nullptr, st, name)) return rc;
  const int seg = topn_max == TOPN_MAX ? 1 : sweep_segments(topn);
  const int rc = with_k_steps(d, [&](auto ks) {
    constexpr int KS = decltype(ks)::value;
    return seg == 1 ? launch_dot_pass<KS, 1>(a, st, name) : seg == 2 ? launch_dot_pass<KS, 2>(a, st, name) : launch_dot_pass<KS, 4>(a, st, name);
  });
  return rc ? rc : sweep_merge<true>(a.sw, top_ids, top_scores, st, name);
}

}  // namespace
}  // namespace ktup

using namespace ktup;

extern "C" size_t ktup_eval_dot_topk_workspace_bytes(int d, int64_t nq, int64_t n_items, int topn, int nsplit) {
  (void)d;
  return sweep_workspace_bytes(nq, n_items, topn, TOPN_MAX, nsplit, 0);
}

extern "C" int ktup_eval_dot_topk(const float* U, int64_t ldu, const float* I, int64_t ldi, int d, const int64_t* u_ids, int64_t nq,
                                  int64_t n_items, const float* user_add, const float* item_add, const int64_t* filt_off,
                                  const int32_t* filt_ids, int topn, int nsplit, int32_t* top_ids, float* top_scores, void* ws,
                                  void* stream) {
  return dot_topk("ktup_eval_dot_topk", TOPN_MAX, U, ldu, I, ldi, d, u_ids, nq, n_items, user_add, item_add, filt_off, filt_ids, topn, nsplit,
                  top_ids, top_scores, ws, stream);
}

extern "C" size_t ktup_eval_dot_topk_wide_workspace_bytes(int d, int64_t nq, int64_t n_items, int topn, int nsplit) {
  (void)d;
  return sweep_workspace_bytes(nq, n_items, topn, TOPN_WIDE_MAX, nsplit, 0);
}

extern "C" int ktup_eval_dot_topk_wide(const float* U, int64_t ldu, const float* I, int64_t ldi, int d, const int64_t* u_ids, int64_t nq,
                                       int64_t n_items, const float* user_add, const float* item_add, const int64_t* filt_off,
                                       const int32_t* filt_ids, int topn, int nsplit, int32_t* top_ids, float* top_scores, void* ws,
                                       void* stream) {
  return dot_topk("ktup_eval_dot_topk_wide", TOPN_WIDE_MAX, U, ldu, I, ldi, d, u_ids, nq, n_items, user_add, item_add, filt_off, filt_ids, topn,
                  nsplit, top_ids, top_scores, ws, stream);
}
