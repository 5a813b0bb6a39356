"""FM with the reference's class surface (jTransUP/models/fm.py): global bias + user bias + item bias + u . i.  The pair term is
K1 (the BPRMF row-dot kernel) and the all-item form K11 (the fp32 MFMA GEMM); the three bias terms are broadcast adds."""
import torch
import torch.nn as nn

from jTransUP.hip import ops
from jTransUP.models._init import GradToggle, make_embedding, xavier_table
from jTransUP.utils.misc import to_gpu


def build_model(FLAGS, user_total, item_total, entity_total, relation_total, i_map=None, e_map=None, new_map=None):
    return FM(FLAGS.embedding_size, user_total, item_total)


class BiasTable(nn.Module):
    """The reference keeps its biases as nn.Embedding(n, 1) whose weight is replaced by a 1-D Parameter of n zeros (fm.py:31-44):
    state-dict key `<name>.weight`, shape (n,).  Same key, same shape; a lookup is an index."""

    def __init__(self, n):
        super(BiasTable, self).__init__()
        self.weight = nn.Parameter(torch.zeros(n, dtype=torch.float32))

    def forward(self, ids):
        return self.weight[ids]


class FM(nn.Module, GradToggle):
    def __init__(self, embedding_size, user_total, item_total):
        super(FM, self).__init__()
        self.embedding_size = embedding_size
        self.user_total = user_total
        self.item_total = item_total
        self.is_pretrained = False
        user_weight = xavier_table(user_total, embedding_size)
        item_weight = xavier_table(item_total, embedding_size)
        self.user_embeddings = to_gpu(make_embedding(user_weight))
        self.item_embeddings = to_gpu(make_embedding(item_weight))
        self.user_bias = to_gpu(BiasTable(user_total))
        self.item_bias = to_gpu(BiasTable(item_total))
        self.bias = nn.Parameter(to_gpu(torch.zeros(1, dtype=torch.float32)))

    def forward(self, u_ids, i_ids):
        """fm.py:58-67: y = b + b_u + b_i + u . i  (the row dot is K1)."""
        dot = ops.score_bprmf(self.user_embeddings.weight, self.item_embeddings.weight, u_ids, i_ids)
        return self.bias + self.user_bias(u_ids) + self.item_bias(i_ids) + dot

    def evaluate(self, u_ids):
        """fm.py:69-80: (len(u), item_total); the GEMM is K11."""
        gemm = ops.eval_bprmf(self.user_embeddings.weight, self.item_embeddings.weight, u_ids)
        return gemm + (self.bias + self.user_bias(u_ids))[:, None] + self.item_bias.weight[None, :]

    topk_descending = True                 # a higher score ranks first (the drivers' eval_descending for this model)

    def evaluate_topk(self, u_ids, items, topn, filt_off=None, filt_ids=None):
        """`evaluate` + the filtered top-n for a whole evaluation pass in one sweep (this build), no (users x items) matrix: the
        user-side and item-side bias terms are formed by torch exactly as `evaluate` forms them and added to the dot product in its
        order, so scores and order are the per-batch route's bits.  `items` is unused; None where the sweep declines."""
        sweep = ops.topk_sweep_for(topn, ops.eval_dot_topk, ops.eval_dot_topk_wide, 'dot')
        if sweep is None:
            return None
        with torch.no_grad():
            user_add = self.bias + self.user_bias(u_ids)
            return sweep(self.user_embeddings.weight, self.item_embeddings.weight, u_ids, topn, filt_off, filt_ids,
                         user_add=user_add, item_add=self.item_bias.weight)

    def rank_items(self, u_ids, items, gold_off, gold_ids, filt_off=None, filt_ids=None):
        """The filtered rank of every gold item of every user of `u_ids` in one sweep (ops.eval_dot_ranks), with the tables and the
        bias terms evaluate_topk passes: gold_ranks on its score bits, no (users x items) matrix.  `items` is unused.  -> int32
        [len(gold_ids)], -1 for a gold that is itself filtered; None where the sweep declines (the caller keeps the matrix route)."""
        with torch.no_grad():
            user_add = self.bias + self.user_bias(u_ids)
            return ops.eval_dot_ranks(self.user_embeddings.weight, self.item_embeddings.weight, u_ids, gold_off, gold_ids, filt_off, filt_ids,
                                      user_add=user_add, item_add=self.item_bias.weight)
