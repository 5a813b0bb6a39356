"""TransD with the reference's class surface (jTransUP/models/transD.py), scored by HIP kernels.

The reference's class is called TransHModel (a copy-paste leftover in transD.py:17); here it is TransDModel, and
`TransHModel = TransDModel` is exported for code that asks this module for the reference's name.  type(model).__name__ is
'TransDModel', so the dispatches on the real TransH ('TransHModel', `norm_embeddings`) never take a TransD model."""
import torch
import torch.nn as nn

from jTransUP.hip import ops
from jTransUP.models._init import GradToggle, make_embedding, xavier_table
from jTransUP.utils.misc import to_gpu


def build_model(FLAGS, user_total, item_total, entity_total, relation_total, i_map=None, e_map=None, new_map=None):
    model_cls = TransHModel
    return model_cls(L1_flag=FLAGS.L1_flag, embedding_size=FLAGS.embedding_size, ent_total=entity_total,
                     rel_total=relation_total)


class TransDModel(nn.Module, GradToggle):
    def __init__(self, L1_flag, embedding_size, ent_total, rel_total):
        super(TransDModel, self).__init__()
        self.L1_flag = L1_flag
        self.embedding_size = embedding_size
        self.ent_total = ent_total
        self.rel_total = rel_total
        self.is_pretrained = False
        ent_weight = xavier_table(ent_total, embedding_size)
        rel_weight = xavier_table(rel_total, embedding_size)
        ent_proj_weight = torch.zeros(ent_total, embedding_size, dtype=torch.float32)      # transD.py:37-38
        rel_proj_weight = torch.zeros(rel_total, embedding_size, dtype=torch.float32)
        self.ent_embeddings = to_gpu(make_embedding(ent_weight))
        self.rel_embeddings = to_gpu(make_embedding(rel_weight))
        self.ent_proj_embeddings = to_gpu(make_embedding(ent_proj_weight, normalize=False))
        self.rel_proj_embeddings = to_gpu(make_embedding(rel_proj_weight, normalize=False))

    def _tables(self):
        return (self.ent_embeddings.weight, self.rel_embeddings.weight, self.ent_proj_embeddings.weight,
                self.rel_proj_embeddings.weight)

    def forward(self, h, t, r):
        """h_perp + r - t_perp with e_perp = e + (e . e_p) r_p (transD.py:61-76)."""
        E, R, Ep, Rp = self._tables()
        return ops.score_transd(E, R, Ep, Rp, h, t, r, self.L1_flag)

    def evaluateHead(self, t, r):
        """transD.py:78-105: every entity projected with the QUERY entity's projection row and the relation's."""
        E, R, Ep, Rp = self._tables()
        return ops.eval_transd(E, R, Ep, Rp, t, r, self.L1_flag, head=True)

    def evaluateTail(self, h, r):
        """transD.py:107-134.  The reference raises NameError here: line 127 names `t_proj_expand`, which that function never
        defines.  Two lines above it builds `h_proj_expand` (the query's own projection row, as evaluateHead uses t's) and never
        uses it; that is the evident intent and what this computes."""
        E, R, Ep, Rp = self._tables()
        return ops.eval_transd(E, R, Ep, Rp, h, r, self.L1_flag, head=False)

    def rank_entities(self, q, r, head, descending, gold_off, gold_ids, filt_off=None, filt_ids=None):
        """A whole evaluateHead / evaluateTail pass + the filtered gold ranks of utils/misc.py:125-146 in one call."""
        E, R, Ep, Rp = self._tables()
        return ops.eval_kg_ranks_transd(E, R, Ep, Rp, q, r, self.L1_flag, head, descending, gold_off, gold_ids, filt_off, filt_ids)

    def predict_entities(self, q, r, head, topn, filt_off=None, filt_ids=None, with_scores=False):
        """The `topn` unfiltered entities nearest to every key -- tails of (q, r, ?) or, with `head`, heads of (?, r, q) -- ascending
        distance, ties -> lower id: int32 (len(q), topn), -1 padded [, their scores].  One sweep without the score matrix
        (ops.eval_kg_topk_transd) up to topn 64 and d 256, the chunked matrix + ops.topk_filtered beyond."""
        E, R, Ep, Rp = self._tables()
        return ops.predict_kg_entities_transd(E, R, Ep, Rp, q, r, self.L1_flag, head, topn, filt_off, filt_ids, with_scores=with_scores)


TransHModel = TransDModel      # the reference's name for this class (transD.py:17)
