/* libktup_hip.so -- TransD extension of the C ABI in ktup_hip.h (same library, same conventions).
 *
 * TransD is the reference's jTransUP/models/transD.py (its class is called TransHModel there, a copy-paste leftover) with the
 * projection of jTransUP/utils/misc.py:36-37 (projection_transD_pytorch_samesize):
 *     e_perp = e + (e . e_p) r_p
 * Four tables, all d wide: E (ent_embeddings), R (rel_embeddings), Ep (ent_proj_embeddings), Rp (rel_proj_embeddings).
 *
 * The entry points live in their own header, and their kernels under csrc/transd/, because the committed kernel profiles are
 * stamped with a hash of csrc/*.hip, csrc/*.h and ktup_hip.h: the profiled kernels stay byte-identical translation units.  The
 * two headers are to be merged when the profiles are next collected.
 *
 * Conventions are those of ktup_hip.h: device pointers, row pitches `ld*` in ELEMENTS, int64 index arrays, `stream` a
 * hipStream_t passed as void*, caller-owned outputs and scratch, gradients ACCUMULATED with atomics into caller-zeroed buffers
 * (a gradient buffer has its table's pitch), 0 on success / KTUP_ERR_* with ktup_last_error() holding the message.
 */
#ifndef KTUP_TRANSD_H
#define KTUP_TRANSD_H

#include "ktup_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------------------------ TransD score  transD.py:61-76
 * score[i] = dist( h_perp + r - t_perp ),  dist = sum |.| (l1) or sum (.)^2.  Any d >= 1, any pitches.                     */
int ktup_score_transd_fwd(const float* E, int64_t lde, const float* R, int64_t ldr, const float* Ep, int64_t ldep,
                          const float* Rp, int64_t ldrp, int d, const int64_t* h, const int64_t* t, const int64_t* r,
                          int64_t n, int l1, float* score, void* stream);
/* autograd of the above (torch.abs differentiates to sign with sign(0) = 0):  with v = h_perp + r - t_perp, g = gscore dist'(v),
 * alpha = h.h_p, beta = t.t_p, gamma = g.r_p:
 *   gE[h] += g + gamma h_p    gEp[h] += gamma h    gE[t] += -g - gamma t_p    gEp[t] += -gamma t
 *   gR[r] += g                gRp[r] += (alpha - beta) g                                                                    */
int ktup_score_transd_bwd(const float* E, int64_t lde, const float* R, int64_t ldr, const float* Ep, int64_t ldep,
                          const float* Rp, int64_t ldrp, int d, const int64_t* h, const int64_t* t, const int64_t* r,
                          int64_t n, int l1, const float* gscore, float* gE, float* gR, float* gEp, float* gRp, void* stream);

/* ------------------------------------------------------------------ all-entity scores  transD.py:78-134
 * out[i * ldo + j] = dist( c_i - e_j - (e_j . a_i) b_i ),  e_j = row j of the candidate table C (normally E, or a slice of it),
 * a_i = Ep[q[i]] (EVERY candidate is projected with the QUERY entity's projection vector, transD.py:94-98), b_i = Rp[r[i]],
 * c_i = q_perp - r (head != 0, evaluateHead) or q_perp + r (evaluateTail; the reference names an undefined t_proj_expand at
 * transD.py:127 and raises NameError -- the h_proj_expand it computes two lines above is what is implemented here).
 * Squared L2 at d in {20, 36, 64, 100, 128} with 16-byte aligned candidate rows runs on the matrix cores (option "eval_mc" = 0:
 * the pair kernel); L1 and every other width take the pair kernel.  ws: ktup_eval_transd_workspace_bytes(d, nq) bytes, 16-byte
 * aligned.                                                                                                                  */
size_t ktup_eval_transd_workspace_bytes(int d, int64_t nq);
int ktup_eval_transd_scores(const float* E, int64_t lde, const float* Ep, int64_t ldep, const float* R, int64_t ldr,
                            const float* Rp, int64_t ldrp, int d, const float* C, int64_t ldc, int64_t n_cand,
                            const int64_t* q, const int64_t* r, int64_t nq, int l1, int head, float* out, int64_t ldo,
                            float* ws, void* stream);

/* ------------------------------------------------------------------ a whole link-prediction pass
 * knowledge_representation.py:93-146 + utils/misc.py:61-146 for TransD; the contract of ktup_eval_kg_ranks (ktup_hip.h): all nq
 * keys at once, CSR gold / filter lists with ABSOLUTE offsets (nq + 1 entries), `chunk` keys scored at a time into `ws`
 * (ktup_eval_kg_ranks_transd_workspace_bytes) and ranked by ktup_eval_gold_ranks; ranks[g] = filtered 0-based rank of gold entry g,
 * -1 for a gold id that is itself filtered.                                                                                 */
size_t ktup_eval_kg_ranks_transd_workspace_bytes(int d, int64_t n_cand, int64_t chunk);
int ktup_eval_kg_ranks_transd(const float* E, int64_t lde, const float* Ep, int64_t ldep, const float* R, int64_t ldr,
                              const float* Rp, int64_t ldrp, int d, const float* C, int64_t ldc, int64_t n_cand,
                              const int64_t* q, const int64_t* r, int64_t nq, int l1, int head, int descending,
                              const int64_t* filt_off, const int32_t* filt_ids, const int64_t* gold_off,
                              const int32_t* gold_ids, int32_t* ranks, int64_t chunk, void* ws, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* KTUP_TRANSD_H */
