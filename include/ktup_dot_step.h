/* libktup_hip.so -- training step of the inner-product recommenders: extension of the C ABI in ktup_hip.h (same library, same
 * conventions).
 *
 * The rec step of FM (fm.py:58-67), coFM (cofm.py:99-108) and CKE (CKE.py:122-135) -- and of BPRMF, which is the same thing without
 * the options -- is one computation: the inner product of a user row with an item-side row, optional bias terms, the BPR loss
 * over (positive, negative) pairs and the gradients back into the gathered rows.  ktup_train_dot_step does all of it in ONE launch
 * (ktup_optim_clip_step follows, as after ktup_train_rec_step / ktup_train_kg_step); ktup_reg_align_pairs is the alignment term of
 * the joint baselines (knowledgable_recommendation.py:385-390, utils/loss.py:33-38 pNormLoss) on the device.
 *
 * The entry points live in their own header, and their kernels under csrc/dotstep/, for the reason ktup_dot.h gives: the committed
 * kernel profiles are stamped with a hash of the .hip and .h files directly under csrc/ and of ktup_hip.h.
 *
 * Conventions are those of ktup_hip.h: device pointers, row pitches `ld*` in ELEMENTS, int64 index arrays, `stream` a
 * hipStream_t passed as void*, caller-owned outputs, 0 on success / KTUP_ERR_* with ktup_last_error() holding the message.
 */
#ifndef KTUP_DOT_STEP_H
#define KTUP_DOT_STEP_H

#include "ktup_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------------------------ the rec step of FM / coFM / CKE (/ BPRMF) in one launch
 * u_ids = [u ; u] and i_ids = [pos ; neg], 2B entries each (the layout ktup_feed_rec fills): rows k and k + B are the positive
 * and the negative pair of example k; only the first B entries of u_ids are read.  For each of the 2B pairs
 *     s = ((gbias[0] + bu[u]) + bi[i]) + dot(U[u], V(i)),     V(i) = I[i]   or   I[i] + X[x_of_item[i]]
 * (the additions of fm.py:45 / cofm.py:45 in their order; the second form is CKE.py:63).  Each of gbias, bu, bi and X may be NULL:
 * the term is then absent.  X needs x_of_item (int64, one entry per row of I) and the other way round.
 *     loss[0] += up * mean_k( -logsigmoid(target * (s_pos[k] - s_neg[k])) )        (evaluated as max(-x, 0) + log1p(exp(-|x|)))
 * and with g_k the derivative of that term with respect to s_pos[k] (-g_k is the one with respect to s_neg[k]) the gradients
 * are ADDED (float atomics; duplicate users and items in a batch are fine) to buffers with the pitches of their tables:
 *     gU[u] += g (V(pos) - V(neg))                 one row add per example: a user is shared by its positive and its negative
 *     gI[pos] += g U[u],   gI[neg] -= g U[u]
 *     gX[x_of_item[pos]] += g U[u],  gX[x_of_item[neg]] -= g U[u]      except for row x_pad: the gradient-free padding row of
 *                                                                      nn.Embedding(padding_idx) is never written
 *     gbi[pos] += g,  gbi[neg] -= g                (gbi may be NULL although bi is given)
 * The gradients of bu and gbias are g + (-g): identically zero under a BPR loss, hence no arguments.  `up`: upstream scalar of the
 * loss (1 / world for data-parallel replicas).
 *
 * Any B >= 1 and 1 <= d <= 256; rows that are 16-byte aligned with d % 4 == 0 (pointers and pitches of every table and gradient)
 * are loaded as float4, others element by element.  Larger d, or the library option "deterministic" being set (the row adds are
 * float atomics issued by many workgroups), is KTUP_ERR_UNSUPPORTED: the caller keeps its multi-launch route.
 * ktup_train_dot_step_supported(d): 1 if a launch with this width would be taken (no launch is made), else 0.                  */
int ktup_train_dot_step_supported(int d);
int ktup_train_dot_step(const float* U, int64_t ldu, const float* I, int64_t ldi, const float* X, int64_t ldx,
                        const int64_t* x_of_item, int64_t x_pad, const float* gbias, const float* bu, const float* bi, int d,
                        const int64_t* u_ids, const int64_t* i_ids, int64_t B, float target, float up, float* loss, float* gU,
                        float* gI, float* gX, float* gbi, void* stream);

/* ------------------------------------------------------------------ alignment term of the joint baselines
 *     loss[0] += scale * mean_{k < n}( sum_j |A[a_ids[k]][j] - B[b_ids[k]][j]| )            (l1 != 0; else the squared differences)
 * and the gradients of that term are ADDED to gA (pitch lda) and gB (pitch ldb): scale / n * sign(a - b) with sign(0) = 0, as
 * torch.abs differentiates, or scale / n * 2 (a - b); gB takes the negative.
 * n is read from DEVICE memory (*n_dev, one int64): the id lists live in fixed buffers of capacity `cap`, so a captured graph
 * replays with a different list length every step.  The kernel clamps n to cap.  n_host: the same length where the host knows it,
 * else -1; n_host > cap is KTUP_ERR_INVALID_ARG.
 * n == 0 adds NOTHING (loss and gradients untouched).  The autograd route's mean over an empty list is NaN there, as the
 * reference's; that is deliberately not reproduced.
 * Any d >= 1, any pitches, duplicate ids allowed.                                                                              */
int ktup_reg_align_pairs(const float* A, int64_t lda, const float* B, int64_t ldb, int d, const int64_t* a_ids,
                         const int64_t* b_ids, const int64_t* n_dev, int64_t n_host, int64_t cap, int l1, float scale, float* loss,
                         float* gA, float* gB, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* KTUP_DOT_STEP_H */
