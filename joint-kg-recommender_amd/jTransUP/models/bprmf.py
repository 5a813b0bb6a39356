"""BPRMF with the reference's class surface (jTransUP/models/bprmf.py), scored by HIP kernels."""
import torch.nn as nn

from jTransUP.hip import ops
from jTransUP.models._init import GradToggle, make_embedding, xavier_table
from jTransUP.utils.misc import to_gpu


def build_model(FLAGS, user_total, item_total, entity_total, relation_total, i_map=None, e_map=None, new_map=None):
    return BPRMF(FLAGS.embedding_size, user_total, item_total)


class BPRMF(nn.Module, GradToggle):
    def __init__(self, embedding_size, user_total, item_total):
        super(BPRMF, self).__init__()
        self.embedding_size = embedding_size
        self.user_total = user_total
        self.item_total = item_total
        self.is_pretrained = False
        user_weight = xavier_table(user_total, embedding_size)
        item_weight = xavier_table(item_total, embedding_size)
        self.user_embeddings = to_gpu(make_embedding(user_weight))
        self.item_embeddings = to_gpu(make_embedding(item_weight))

    def forward(self, u_ids, i_ids):
        """K1: score[b] = U[u_b] . I[i_b]   (bprmf.py:46-49)."""
        return ops.score_bprmf(self.user_embeddings.weight, self.item_embeddings.weight, u_ids, i_ids)

    def evaluate(self, u_ids):
        """K11: all-item scores U[u] . I^T (bprmf.py:51-54)."""
        return ops.eval_bprmf(self.user_embeddings.weight, self.item_embeddings.weight, u_ids)

    topk_descending = True                 # a higher score ranks first (the drivers' eval_descending for this model)

    def evaluate_topk(self, u_ids, items, topn, filt_off=None, filt_ids=None):
        """K11 + K17 for a whole evaluation pass in one sweep (this build): filtered top-n item ids of every user of `u_ids`
        without the (users x items) matrix; the scores and the order are `evaluate`'s + topk_filtered's, bit for bit.  `items` is
        unused (this model has no prepared item side); None where the sweep declines (embedding_size > 256; topn > 16 unless the
        wide lists serve it, ops.topk_sweep_for)."""
        sweep = ops.topk_sweep_for(topn, ops.eval_dot_topk, ops.eval_dot_topk_wide, 'dot')
        return sweep and sweep(self.user_embeddings.weight, self.item_embeddings.weight, u_ids, topn, filt_off, filt_ids)

    def rank_items(self, u_ids, items, gold_off, gold_ids, filt_off=None, filt_ids=None):
        """The filtered rank of every gold item of every user of `u_ids` in one sweep (ops.eval_dot_ranks): gold_ranks on `evaluate`'s
        scores without the (users x items) matrix, on evaluate_topk's score bits.  `items` is unused.  -> int32 [len(gold_ids)], -1 for
        a gold that is itself filtered; None where the sweep declines (the caller keeps the matrix route)."""
        return ops.eval_dot_ranks(self.user_embeddings.weight, self.item_embeddings.weight, u_ids, gold_off, gold_ids, filt_off, filt_ids)
