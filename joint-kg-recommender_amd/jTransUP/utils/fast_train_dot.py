"""GPU-resident training steps of the inner-product recommenders: FM (item_recommendation.py:160-195 -> DotRecStepper) and the joint
baselines coFM, CKE and CFKG (knowledgable_recommendation.py:330-401 -> BaselineJointStepper), on the machinery of utils/fast_train.py
(flat gradient bucket, data-parallel slice + all-reduce, pre-bound launches, HIP-graph replay, the K20 clip + step).

Their rec step is one computation -- the inner product of a user row with an item-side row, optional bias terms, the BPR loss, the
gradients back into the gathered rows -- and ONE launch: ktup_train_dot_step (include/ktup_hip.h), followed by
ktup_optim_clip_step.  The kg side takes what exists: ktup_train_kg_step (TransE) for coFM, the TransR launches of KGStepper for
CKE.  coFM with its own item table adds the alignment term of knowledgable_recommendation.py:385-390 to EVERY step:
ktup_reg_align_pairs, whose id lists the host builds exactly as the autograd route does (getMappedEntities / getMappedItems on the
global batch) and copies, with their length, into fixed buffers outside the graph -- or, on a device-fed step, ktup_feed_align_lists
builds in those buffers from the batch the feed launch drew.  CFKG's rec step is a translation, not an
inner product (user + buy - item-entity, CFKG.py:66-80): ONE launch of its own, ktup_train_cfkg_rec_step; its kg step is coFM's.

Device-fed steps (-device_sampling, `attach_feeds` + `set_id_maps`): feed launch -> [ktup_feed_remap_ids: raw ids -> rows of the joint
table, coFM -share_embeddings and CFKG] -> step launch -> [ktup_feed_align_lists + ktup_reg_align_pairs, coFM with its own item table]
-> clip + optimizer launch, one graph per step kind and one per cycle of steps (`fed_step`, `fed_cycle` of utils/fast_train.py).

rec step:  bprLoss(pos, neg, target)                                                   [+ norm_lambda * pNormLoss(ent rows, item rows)]
kg step:   kg_lambda * (marginLoss(pos, neg, margin) + normLoss(ent rows) + normLoss(rel rows))     [+ the same alignment term]
"""
import torch

from jTransUP.hip import lib as L
from jTransUP.utils import step_plans as plans
from jTransUP.utils.fast_train import _StepperBase, _p


def cfkg_step_supported(d):
    """Whether ktup_train_cfkg_rec_step takes this width (and the library option `deterministic` is off): the driver's condition."""
    return bool(L.load().ktup_train_cfkg_rec_step_supported(int(d)))


def dot_step_supported(d):
    """Whether ktup_train_dot_step takes this width (and the library option `deterministic` is off): the drivers' condition."""
    return bool(L.load().ktup_train_dot_step_supported(int(d)))


class DotRecStepper(_StepperBase):
    """FM: tables U, I, the two bias tables and the global bias; a step is ktup_train_dot_step + the optimizer launch.
    loss slot 0: bpr.  The gradients of the user bias and the global bias are identically zero under a BPR loss (g - g): their
    buffers stay zero-filled, and the optimizer applies its weight decay to them as on the autograd route.  A model without bias
    tables (BPRMF) takes the same launch without the options (tools/dot_step_time.py; the drivers keep RecStepper for it)."""
    KINDS = ('rec',)
    N_IDS = {'rec': 3}

    def _setup(self, FLAGS, f32, i64):
        m = self.m
        self.tabs = (m.user_embeddings.weight, m.item_embeddings.weight)
        if hasattr(m, 'user_bias'):
            self.tabs += (m.user_bias.weight, m.item_bias.weight, m.bias)
        if not dot_step_supported(self.tabs[0].shape[1]):
            raise L.KtupError('ktup_train_dot_step does not take embedding_size %d (or KTUP_DETERMINISTIC=1 is set)' % self.tabs[0].shape[1])
        self._id_buffers('rec', i64)
        self.fused_step = True

    def _bind(self, st):
        U, I = self.tabs[:2]
        bu, bi, gb = self.tabs[2:] if len(self.tabs) > 2 else (None, None, None)
        self.fused_step = True
        self._rec_fused = plans.dot_step(U, I, self.rec_ids, self.B, self.target, 1.0 / self.world, self.loss, self._g, st,
                                         bias=(gb, bu, bi))

    def _rec_launches(self):
        self._rec_fused()
        self._optimizer_launches(loss=(_p(self.loss), 1, 1.0, _p(self.out['rec']), self._acc_ptr('rec')))
        return self.out['rec']


class BaselineJointStepper(_StepperBase):
    """coFM (either setting of -share_embeddings), CKE and CFKG (whose item table IS the entity table: no alignment term).

    A table joins the optimizer step with the first step that can give it a gradient, as on the autograd route, where a
    parameter's `.grad` is None until its first backward and the optimizer skips it until then (no weight decay, no moment decay,
    Adam's step count starts later): the relation table (and CKE's projections) wait for the first kg step, the user side for the
    first rec step.  Until then their gradient views are kept aside; waking a table drops the captured graphs.

    loss slots: rec 0 bpr | kg 0 margin, 2 normLoss(ent rows), 3 normLoss(rel rows) | 6 the alignment term (already scaled)."""
    KINDS = ('rec', 'kg')
    N_IDS = {'rec': 3, 'kg': 6}
    ALIGN_SLOT = 6
    READOPT_GRADS = False       # a sleeping table's `.grad` stays None through the all-reduce

    def _setup(self, FLAGS, f32, i64):
        m, B = self.m, self.B
        self.kg_lambda, self.norm_lambda = float(FLAGS.kg_lambda), float(FLAGS.norm_lambda)
        self.cke = hasattr(m, 'proj_embeddings')
        self.cfkg = not self.cke and not hasattr(m, 'user_bias')       # tables (U, E, R): the rec score is a translation
        U, E, R = m.user_embeddings.weight, m.ent_embeddings.weight, m.rel_embeddings.weight
        I = m.item_embeddings.weight                                    # coFM -share_embeddings: the entity table itself
        d = U.shape[1]
        if not (cfkg_step_supported(d) if self.cfkg else dot_step_supported(d)):
            raise L.KtupError('%s does not take embedding_size %d (or KTUP_DETERMINISTIC=1 is set)'
                              % ('ktup_train_cfkg_rec_step' if self.cfkg else 'ktup_train_dot_step', d))
        self.lam = torch.full((), self.kg_lambda, **f32)               # upstream gradient of the multi-launch kg terms
        self._id_buffers('rec', i64); self._id_buffers('kg', i64)
        if self.cke:
            M = m.proj_embeddings.weight
            self.tabs = (U, I, E, R, M)
            touch = {'rec': (U, I, E), 'kg': (E, R, M)}
            # the kg step as ONE launch (ktup_train_transr_step); KTUP_FUSED_STEP=0, or a shape it does not take, keeps the bucketed route
            self.transr_step = bool(self.want_fused and L.load().ktup_train_transr_step_supported(d)
                                    and 1 <= B <= 4096 and 1 <= min(R.shape[0], M.shape[0]) <= 4096)
            self.rws = None
            if not self.transr_step:                                    # scratch of the relation-bucketed forward
                nbytes = L.load().ktup_score_transr_workspace_bytes(2 * B, R.shape[0])
                self.rws = torch.empty((nbytes + 3) // 4, dtype=torch.int32, device=self.dev)
            self.align = False
            self.fused_step = False                                     # (`can_feed` decides per kind here, not `_feedable`)
            # The HOST-FED kg step is never captured: the relation-bucketed TransR kernels (d = 64, 100, 128) clear their counters in the
            # workspace with hipMemsetAsync, and a captured memset node whose destination lies inside a pooled allocation writes garbage
            # from its second replay on -- the bucket kernels then index past the workspace.  The rec step replays.
            # (With `transr_step` the kg step is ktup_train_transr_step, which has no memset and replays safely; it is still
            # issued eagerly here because the suite pins this stepper's graphs to {'rec'}; the device-fed kg step is captured, `_fed`.)
            self.never_captured = frozenset(['kg'])
        elif self.cfkg:
            if I is not E:
                raise L.KtupError('CFKG scores items on the entity table (-share_embeddings is forced)')
            self.tabs = (U, E, R)
            touch = {'rec': (U, E, R), 'kg': (E, R)}                    # the buy relation is a row of R: R wakes with either kind
            self.align = False
            self.kg_fused = bool(self.want_fused and L.load().ktup_train_step_supported(2, d, 0))
            self.fused_step = False
        else:
            bu, bi, gb = m.user_bias.weight, m.item_bias.weight, m.bias
            shared = I is E
            self.tabs = (U, bu, bi, gb, R, E) + (() if shared else (I,))
            self.align = not shared                                     # :385-390, coFM with its own item table
            touch = {'rec': (U, I, bu, bi, gb) + ((E,) if self.align else ()), 'kg': (E, R) + ((I,) if self.align else ())}
            self.kg_fused = bool(self.want_fused and L.load().ktup_train_step_supported(2, d, 0))
            self.fused_step = False
        self.remaps = self.cfkg or (not self.cke and I is E)             # the step kernels read rows of the joint table
        self.id_rows = {}                                               # kind -> raw id -> joint row (int64, device; None: a gap)
        self.partner = {}                                               # kind -> raw id -> aligned id of the other space, or -1
        self._align_lists = {}
        self._touch = touch
        self._views = {id(t): t.grad for t in self.tabs}                # ReplicaGradSync's views into the flat bucket
        self._awake = set()
        for t in self.tabs:
            t.grad = None
        if self.align:
            # [n | entity ids (cap) | item ids (cap)]: a kg step lists up to 4 x GB distinct entities, a rec step up to 2 x GB items
            self.al_cap = 4 * self.GB
            self._al = torch.zeros(1 + 2 * self.al_cap, **i64)
            self._al_host = torch.zeros(1 + 2 * self.al_cap, dtype=torch.int64).pin_memory()      # staging, filled in place
            self._al_np = self._al_host.numpy()
            self._al_copied = torch.cuda.Event()
            self.total = {k: torch.zeros((), **f32) for k in self.KINDS}

    # ------------------------------------------------------------------------------------------------ late tables
    def _g(self, t):
        """A sleeping table's `.grad` is None: the launch plans write into, and `_plans` keys on, its view of the flat bucket."""
        return self._views[id(t)].data_ptr()

    def _wake(self, kind):
        new = [t for t in self._touch[kind] if id(t) not in self._awake]
        if not new:
            return
        for t in new:
            t.grad = self._views[id(t)]
            self._awake.add(id(t))
        torch.cuda.current_stream(self.dev).synchronize()               # a replay may still be running (at most twice per run)
        self._graphs = {}                                               # captured with the shorter table list of the optimizer launch
        self._eager_steps = {k: 0 for k in self.KINDS}
        self._keys = None
        self.trainer.fused._plan = None

    # ------------------------------------------------------------------------------------------------ device-fed steps
    def set_id_maps(self, i_map, e_map, ikg_map, n_items=None, n_ent=None):
        """The run's id maps (load_kg_rating_data.load_data: i_map / e_map = raw item / entity id -> index of the joint vocabulary,
        ikg_map = index -> (entity id or -1, item id or -1)) as device tables, once per run:
        `id_rows[kind]`  raw id -> row of the joint table (coFM -share_embeddings, CFKG; what `[i_map[i] for i in ...]` does per step),
        `partner[kind]`  raw id -> the aligned id of the other space or -1 (coFM with its own item table; getMappedEntities /
                         getMappedItems per step).
        kind 'rec' is keyed by item ids, 'kg' by entity ids.  An id in [0, n) without a joint row leaves `id_rows[kind]` None: the
        kind is not fed (the host route raises KeyError on such an id)."""
        i64 = dict(dtype=torch.int64, device=self.dev)
        sizes = {'rec': len(i_map) if n_items is None else int(n_items), 'kg': len(e_map) if n_ent is None else int(n_ent)}
        maps = {'rec': i_map, 'kg': e_map}
        self.id_rows, self.partner = {}, {}
        if self.remaps:
            rows_total = self.m.ent_embeddings.weight.shape[0]
            for kind, mp in maps.items():
                rows = [mp.get(x, -1) for x in range(sizes[kind])]
                if any(not isinstance(r, int) or r < 0 for r in rows):
                    self.id_rows[kind] = None
                    continue
                if max(rows) >= rows_total:
                    raise L.KtupError('%s id map points at row %d of a table of %d rows' % (kind, max(rows), rows_total))
                self.id_rows[kind] = torch.tensor(rows, **i64)
        if self.align:
            limit = {'rec': self.m.ent_embeddings.weight.shape[0], 'kg': self.m.item_embeddings.weight.shape[0]}
            for kind, mp in maps.items():
                mine, other = (1, 0) if kind == 'rec' else (0, 1)      # position of the id's own space / its partner's in a pair
                out, ok = [], True
                for x in range(sizes[kind]):
                    pair = ikg_map[mp[x]] if x in mp else None
                    out.append(-1 if pair is None else int(pair[other]))
                    # the lists the host builds carry the pair's own id of x; it is x itself in every vocabulary load_data builds
                    ok = ok and (pair is None or pair[other] == -1 or pair[mine] == x)
                if out and max(out) >= limit[kind]:
                    raise L.KtupError('%s alignment map points at row %d of a table of %d rows' % (kind, max(out), limit[kind]))
                self.partner[kind] = torch.tensor(out, **i64) if ok else None
        self._feed_ok = {}
        self._keys = None

    def maps_cover(self, kind):
        """Whether `set_id_maps` gave this kind every table its steps need (device-fed or host-driven on the device)."""
        return (not self.remaps or self.id_rows.get(kind) is not None) and (not self.align or self.partner.get(kind) is not None)

    def can_feed(self, kind):
        """Per kind: one process, a step that reads nothing but the [pos ; neg] id arrays the feed launch fills (the rec step always;
        the kg step where it is ONE launch -- the multi-launch sequences read `ht4`), the id tables of `set_id_maps` covering every
        id the sampler draws, and an id count ktup_feed_align_lists takes."""
        ok = self._feed_ok.get(kind)
        if ok is None:
            ok = kind in self._feeds and self.world == 1 and self.maps_cover(kind)
            if ok and kind == 'kg':
                ok = self.transr_step if self.cke else self.kg_fused
            sm = self._sampler
            if ok and self.remaps:
                ok = (sm.n_items if kind == 'rec' else sm.n_ent) <= self.id_rows[kind].numel()
            elif ok:                                                    # raw ids ARE the rows the step kernels read
                ok = sm.n_items <= self.m.item_embeddings.weight.shape[0] if kind == 'rec' else sm.n_ent <= self.m.ent_embeddings.weight.shape[0]
            if ok and self.align:
                n_ids = (2 if kind == 'rec' else 4) * self.B
                ok = n_ids <= self.al_cap and bool(L.load().ktup_feed_align_lists_supported(n_ids))
            ok = self._feed_ok[kind] = bool(ok)
        return ok

    def _make_feed(self, kind, st):
        """The feed launch, then -- where the step kernels read rows of the joint table -- the raw ids it wrote mapped in place."""
        feed = _StepperBase._make_feed(self, kind, st)
        if not (self.remaps and self.can_feed(kind)):
            return feed
        tab = self.id_rows[kind]
        a, b = (self.i2, None) if kind == 'rec' else (self.h2, self.t2)
        remap = L.bind('ktup_feed_remap_ids', _p(tab), tab.numel(), _p(a), a.numel(), None if b is None else _p(b),
                       0 if b is None else b.numel(), _p(self._sampler.fail), st)

        def run():
            feed()
            remap()
        return run

    def _bind_feeds(self, st):
        _StepperBase._bind_feeds(self, st)
        self._align_lists = {}
        if not self.align:
            return
        cap = self.al_cap
        for kind in self._feeds:
            if not self.can_feed(kind):
                continue
            tab = self.partner[kind]
            a, b = (self.i2, None) if kind == 'rec' else (self.h2, self.t2)
            self._align_lists[kind] = L.bind('ktup_feed_align_lists', _p(a), a.numel(), None if b is None else _p(b),
                                             0 if b is None else b.numel(), _p(tab), tab.numel(), int(kind == 'kg'), cap, _p(self._al),
                                             _p(self._al[1:]), _p(self._al[1 + cap:]), None, st)

    def _asleep(self, kind):
        return any(id(t) not in self._awake for t in self._touch[kind])

    def _fed(self, kinds, run, cycle=False):
        if cycle and any(self._asleep(k) for k in kinds):
            # A cycle never wakes a table: waking drops the graphs, so the cycle could not run anyway, and a table must join the
            # optimizer step with the first step of its kind that actually runs -- not when a cycle that holds the kind is asked for
            return 0
        if not cycle:
            self._wake(kinds[0])
        held = self.never_captured
        if self.cke and self.transr_step:
            self.never_captured = frozenset()       # ktup_train_transr_step: no memset, no scratch -- the fed kg step replays
        try:
            return run()
        finally:
            self.never_captured = held

    def fed_step(self, kind):
        return self._fed((kind,), lambda: _StepperBase.fed_step(self, kind))

    def fed_cycle(self, kinds):
        return self._fed(kinds, lambda: _StepperBase.fed_cycle(self, kinds), cycle=True)

    # ------------------------------------------------------------------------------------------------ launch plans
    def _bind(self, st):
        m, B, b, g = self.m, self.B, L.bind, self._g
        inv = 1.0 / self.world
        rec = (self.rec_ids, B, self.target, inv, self.loss, g, st)
        kg = (self.kg_ids, B, self.l1, self.margin)
        seq = (self.score, self.gscore, self.loss, self.lam, g, st)    # the multi-launch kg steps, with kg_lambda as the upstream scalar
        if self.cke:
            U, I, E, R, M = self.tabs
            self._rec_fused = plans.dot_step(U, I, *rec, E=E, i2e=m._item2ent, ent_pad=m.ent_total - 1)
            self._kg = []
            if self.transr_step:
                self._kg_transr = plans.transr_step(E, R, M, *kg, self.kg_lambda, self.loss, g, st)
            else:
                self._kg = plans.kg_sequence('transr', (E, R, M), *kg, *seq, rws=self.rws)
            return
        if self.cfkg:
            U, E, R = self.tabs
            d = U.shape[1]
            self._rec_fused = b('ktup_train_cfkg_rec_step', _p(U), U.stride(0), _p(E), E.stride(0), _p(R), R.stride(0), m.rel_total - 1, d,
                                _p(self.u2), _p(self.i2), B, self.l1, self.target, inv, _p(self.loss), g(U), g(E), g(R), st)
        else:
            U, bu, bi, gb, R, E = self.tabs[:6]
            I = self.tabs[6] if self.align else E
            d = U.shape[1]
            self._rec_fused = plans.dot_step(U, I, *rec, bias=(gb, bu, bi))
        if self.kg_fused:
            self._kg_fused = plans.kg_step(E, R, None, *kg, self.kg_lambda, self.loss, g, None, st)
        # (for a width ktup_train_kg_step does not take, d % 4 != 0)
        self._kg = plans.kg_sequence('transe', (E, R), *kg, *seq)
        if self.align:
            cap = self.al_cap
            # every rank applies the whole term (the lists come from the global batch), scaled 1 / world like the other replicated terms
            self._align = b('ktup_reg_align_pairs', _p(E), E.stride(0), _p(I), I.stride(0), d, _p(self._al[1:]), _p(self._al[1 + cap:]),
                            _p(self._al), -1, cap, self.l1, self.norm_lambda * inv, _p(self.loss[self.ALIGN_SLOT:]), g(E), g(I), st)

    # ------------------------------------------------------------------------------------------------ alignment lists
    def set_alignment(self, e_ids, i_ids):
        """The aligned (entity, item) pairs of the NEXT step (getMappedEntities / getMappedItems on the global batch): copied, with
        their number, into the fixed buffers ktup_reg_align_pairs reads -- one host-to-device copy, outside the graph."""
        n = len(e_ids)
        if n != len(i_ids) or n > self.al_cap:
            raise L.KtupError('%d / %d alignment ids for buffers of %d' % (n, len(i_ids), self.al_cap))
        cap, host = self.al_cap, self._al_np
        self._al_copied.synchronize()                                   # the previous step's copy has left the staging buffer
        host[0] = n
        host[1:1 + n] = e_ids
        host[1 + cap:1 + cap + n] = i_ids
        self._al[:1 + cap + n].copy_(self._al_host[:1 + cap + n], non_blocking=True)
        self._al_copied.record()

    def _finish(self, kind, n_slots, scale):
        """Alignment launch (own item table), optimizer launch, the step's loss."""
        if self.align:
            if self._acc_on:                                            # a fed step: the lists of the batch the feed launch drew
                self._align_lists[kind]()
            self._align()
        self._optimizer_launches(loss=(_p(self.loss), n_slots, scale, _p(self.out[kind]), None if self.align else self._acc_ptr(kind)))
        if not self.align:
            return self.out[kind]
        # the alignment term is not part of what kg_lambda scales: its slot is folded in, and cleared, here
        torch.add(self.out[kind], self.loss[self.ALIGN_SLOT], out=self.total[kind])
        self.loss[self.ALIGN_SLOT:self.ALIGN_SLOT + 1].zero_()
        if self._acc_on:                                                # take_sums: the whole step's loss, alignment term included
            self.acc[kind].add_(self.total[kind])
        return self.total[kind]

    # ------------------------------------------------------------------------------------------------ steps
    def _rec_launches(self):
        self._rec_fused()
        return self._finish('rec', 1, 1.0)

    def _kg_launches(self):
        """One launch where there is one, else the multi-launch sequence: gradients x kg_lambda either way, slots unscaled."""
        if self.cke and self.transr_step:
            self._kg_transr()
        elif not self.cke and self.kg_fused:
            self._kg_fused()
        else:
            for launch in self._kg:
                launch()
        return self._finish('kg', 4, self.kg_lambda)

    def rec_step(self, u, pi, ni, align=None):
        """u, pi, ni: int64 device tensors of the GLOBAL batch (coFM -share_embeddings and CFKG: pi, ni already mapped to entity rows).
        align = (entity ids, item ids), coFM with its own item table only.  Returns the step's loss (0-dim device tensor)."""
        self._wake('rec')
        self._take_alignment(align)
        return self._step('rec', (u, pi, ni))

    def kg_step(self, ph, pt, pr, nh, nt, nr, align=None):
        self._wake('kg')
        self._take_alignment(align)
        return self._step('kg', (ph, pt, pr, nh, nt, nr))

    def _take_alignment(self, align):
        if self.align:
            if align is None:
                raise L.KtupError('coFM with its own item table: every step takes its alignment lists (align=)')
            self.set_alignment(*align)
        elif align is not None and (len(align[0]) or len(align[1])):
            raise L.KtupError('this model has no alignment term')
