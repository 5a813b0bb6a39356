"""CFKG with the reference's class surface (jTransUP/models/CFKG.py): TransE over users, item-entities and relations, with one
extra "buy" relation (the last row of the relation table) between a user and an item -- a thin module over the K2 / K12 kernels,
with the whole rec evaluation pass behind one call (evaluate_topk; the training step: utils/fast_train_dot.py).

Ratings are triples (user, buy, item) whose head lives in the USER table and whose tail in the shared item / entity table
(CFKG.py:62, 66-80).  K2 gathers heads and tails from one table, so the rec branch scores on the row-stack [users ; entities]
(torch.cat -- plumbing; autograd splits the gradient back) with item ids offset by the user count; the all-item evaluation needs
no stacking: K12 takes the query table (users) and the candidate table (entities) separately."""
import torch
import torch.nn as nn

from jTransUP.hip import ops
from jTransUP.models._init import GradToggle, make_embedding, xavier_table
from jTransUP.utils.misc import to_gpu


def build_model(FLAGS, user_total, item_total, entity_total, relation_total, i_map=None, e_map=None, new_map=None):
    return CFKG(L1_flag=FLAGS.L1_flag, embedding_size=FLAGS.embedding_size, user_total=user_total, item_total=item_total,
                entity_total=entity_total, relation_total=relation_total)


class CFKG(nn.Module, GradToggle):
    def __init__(self, L1_flag, embedding_size, user_total, item_total, entity_total, relation_total):
        super(CFKG, self).__init__()
        self.L1_flag = L1_flag
        self.embedding_size = embedding_size
        self.user_total = user_total
        self.item_total = item_total
        self.ent_total = entity_total
        self.rel_total = relation_total + 1           # + the buy relation (CFKG.py:34)
        self.is_pretrained = False
        self.user_embeddings = to_gpu(make_embedding(xavier_table(user_total, embedding_size)))
        ent_weight = xavier_table(entity_total, embedding_size)
        rel_weight = xavier_table(self.rel_total, embedding_size)
        self.ent_embeddings = to_gpu(make_embedding(ent_weight))
        self.rel_embeddings = to_gpu(make_embedding(rel_weight))
        self.item_embeddings = self.ent_embeddings    # shared table (CFKG.py:62)

    def forward(self, ratings, triples, is_rec=True):
        E, R = self.ent_embeddings.weight, self.rel_embeddings.weight
        if is_rec and ratings is not None:
            u_ids, i_ids = ratings
            # CFKG.py:66-80 : user + buy - item-entity, on the batch's rows only (heads = the gathered user rows, tails = the
            # gathered entity rows of one 2B-row table) instead of concatenating the two whole tables per step
            n = u_ids.numel()
            both = torch.cat([self.user_embeddings(u_ids), self.ent_embeddings(i_ids)])
            at = torch.arange(n, device=u_ids.device)
            buy = torch.full_like(u_ids, self.rel_total - 1)
            return ops.score_transe(both, R, at, at + n, buy, self.L1_flag)
        if not is_rec and triples is not None:
            h, t, r = triples
            return ops.score_transe(E, R, h, t, r, self.L1_flag)                                             # CFKG.py:81-92
        raise NotImplementedError

    def evaluateRec(self, u_ids, all_i_ids=None):
        """CFKG.py:100-118: (user + buy) against every (or the given) item-entity row."""
        cand = self.item_embeddings(all_i_ids) if all_i_ids is not None else self.item_embeddings.weight
        buy = torch.full_like(u_ids, self.rel_total - 1)
        return ops.eval_transe(self.user_embeddings.weight, self.rel_embeddings.weight, u_ids, buy, self.L1_flag, head=False,
                               candidates=cand.detach().contiguous())

    topk_descending = False          # evaluate_topk ranks ascending distance (the inner-product models: True)
    topk_takes_candidates = True     # ... and takes the candidates as entity-row ids: the route that serves -share_embeddings

    def evaluate_topk(self, u_ids, items, topn, filt_off=None, filt_ids=None):
        """The whole rec evaluation pass in one sweep (ktup_eval_cfkg_topk): evaluateRec's scores of every user of `u_ids` against
        the entity rows `items` (int64 ids; None = every row) AND their filtered top-n, without the (users x candidates) matrix.
        Ids in the filter lists and in the result are positions in `items`.  -> int32 (len(u_ids), topn), -1 padded, or None where
        the kernel declines the shape (the caller keeps the batch walk)."""
        sweep = ops.topk_sweep_for(topn, ops.eval_cfkg_topk, ops.eval_cfkg_topk_wide, 'cfkg_l1' if self.L1_flag else 'cfkg_l2')
        return sweep and sweep(self.user_embeddings.weight, self.rel_embeddings.weight, self.rel_total - 1, self.item_embeddings.weight,
                               u_ids, topn, self.L1_flag, cand_ids=items, filt_off=filt_off, filt_ids=filt_ids)

    def rank_items(self, u_ids, items, gold_off, gold_ids, filt_off=None, filt_ids=None):
        """The filtered rank of every gold item of every user of `u_ids` in one sweep (ops.eval_cfkg_ranks): gold_ranks(ascending) on
        evaluate_topk's distances -- the same bits -- against the entity rows `items` (int64 ids; None = every row), no (users x
        candidates) matrix.  Gold and filter ids are positions in `items`.  -> int32 [len(gold_ids)], -1 for a gold that is itself
        filtered or has no row; None where the sweep declines (the caller keeps the matrix route)."""
        return ops.eval_cfkg_ranks(self.user_embeddings.weight, self.rel_embeddings.weight, self.rel_total - 1, self.item_embeddings.weight,
                                   u_ids, self.L1_flag, gold_off, gold_ids, cand_ids=items, filt_off=filt_off, filt_ids=filt_ids)

    def _cand(self, all_e_ids):
        return self.ent_embeddings(all_e_ids).detach().contiguous() if all_e_ids is not None else None

    def evaluateHead(self, t, r, all_e_ids=None):
        """CFKG.py:120-138."""
        return ops.eval_transe(self.ent_embeddings.weight, self.rel_embeddings.weight, t, r, self.L1_flag, head=True,
                               candidates=self._cand(all_e_ids))

    def evaluateTail(self, h, r, all_e_ids=None):
        """CFKG.py:140-158."""
        return ops.eval_transe(self.ent_embeddings.weight, self.rel_embeddings.weight, h, r, self.L1_flag, head=False,
                               candidates=self._cand(all_e_ids))

    def rank_entities(self, q, r, head, descending, gold_off, gold_ids, filt_off=None, filt_ids=None, all_e_ids=None):
        """A whole evaluateHead / evaluateTail pass (CFKG.py:120-158) + the filtered gold ranks of utils/misc.py:125-146 in one call
        (K12 + K18 per chunk of 512 keys under the C ABI)."""
        return ops.eval_kg_ranks(self.ent_embeddings.weight, self.rel_embeddings.weight, None, q, r, self.L1_flag, head, descending,
                                 gold_off, gold_ids, filt_off, filt_ids, candidates=self._cand(all_e_ids))

    def predict_entities(self, q, r, head, topn, filt_off=None, filt_ids=None, with_scores=False, all_e_ids=None):
        """The `topn` unfiltered candidates nearest to every key -- tails of (q, r, ?) or, with `head`, heads of (?, r, q) -- ascending
        distance, ties -> lower id: int32 (len(q), topn), -1 padded [, their scores].  The KG score is TransE's and the candidates are
        those of rank_entities; one sweep without the score matrix (ops.eval_kg_topk) up to topn 64 and d 256, the chunked matrix +
        ops.topk_filtered beyond."""
        return ops.predict_kg_entities(self.ent_embeddings.weight, self.rel_embeddings.weight, None, q, r, self.L1_flag, head, topn,
                                       filt_off, filt_ids, candidates=self._cand(all_e_ids), with_scores=with_scores)
