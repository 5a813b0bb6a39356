/* libktup_hip.so -- inner-product evaluation pass: extension of the C ABI in ktup_hip.h (same library, same conventions).
 *
 * The whole-pass evaluation of the inner-product recommenders (BPRMF bprmf.py:51-54, FM fm.py:69-80, CKE CKE.py:142-153 and coFM
 * cofm.py:127-141): all-item scores AND the filtered top-n of every user in one sweep that never writes the (users x items)
 * matrix -- what ktup_eval_bprmf_scores + the bias adds + ktup_eval_topk_filtered(descending) compute batch by batch.
 *
 * The entry points live in their own header, and their kernels under csrc/dot/, because the committed kernel profiles are
 * stamped with a hash of the .hip and .h files directly under csrc/ and of ktup_hip.h: the profiled kernels stay byte-identical
 * translation units.  The headers are to be merged when the profiles are next collected.
 *
 * Conventions are those of ktup_hip.h: device pointers, row pitches `ld*` in ELEMENTS, int64 index arrays, `stream` a
 * hipStream_t passed as void*, caller-owned outputs and scratch, 0 on success / KTUP_ERR_* with ktup_last_error() holding the
 * message.
 */
#ifndef KTUP_DOT_H
#define KTUP_DOT_H

#include "ktup_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------------------------ scores + filtered top-n of a whole pass
 * score(b, j) = (U[u_ids[b]] . I[j] + user_add[b]) + item_add[j]
 * The dot product is the fp32 fma chain over k = 0 .. d-1 starting from +0 (the bits of ktup_eval_bprmf_scores); the two additions
 * are separately rounded fp32 adds in that order, a NULL term is skipped -- the bits of
 *     gemm + (bias + user_bias[u])[:, None] + item_bias[None, :]
 * The ranked list is that of ktup_eval_topk_filtered(scores, descending = 1): descending score, ties -> lower id, ids of the
 * user's filter list skipped, -1 padding; top_scores (may be NULL) holds the scores themselves, 0 in padded slots.
 *
 * Any 1 <= d <= 256 (rows that are not 16-byte aligned or d % 4 != 0 are loaded element by element), any pitches, topn <= 16,
 * n_items < 2^31, duplicates in u_ids allowed; otherwise KTUP_ERR_UNSUPPORTED and the caller keeps the per-batch calls.
 * user_add: nq floats, the term of user b of u_ids; item_add: n_items floats.  filt_off / filt_ids: CSR filter sets per user of
 * u_ids (filt_off[nq + 1]; NULL = none).  nsplit: into how many contiguous parts the catalogue is cut (each part of a block of 64
 * users is one workgroup); 0 = chosen by the library, a larger request than the merge takes (512 / topn, at most 32) or the
 * catalogue yields is reduced.  `ws`: ktup_eval_dot_topk_workspace_bytes bytes for the same arguments, 16-byte aligned.       */
size_t ktup_eval_dot_topk_workspace_bytes(int d, int64_t nq, int64_t n_items, int topn, int nsplit);
int ktup_eval_dot_topk(const float* U, int64_t ldu, const float* I, int64_t ldi, int d, const int64_t* u_ids, int64_t nq,
                       int64_t n_items, const float* user_add, const float* item_add, const int64_t* filt_off,
                       const int32_t* filt_ids, int topn, int nsplit, int32_t* top_ids, float* top_scores, void* ws,
                       void* stream);

#ifdef __cplusplus
}
#endif
#endif /* KTUP_DOT_H */
