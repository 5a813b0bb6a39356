"""GPU-resident training steps of the three drivers: the arithmetic of their `train_loop` step bodies
(knowledgable_recommendation.py:330-401 -> JointStepper; item_recommendation.py:160-195 -> RecStepper;
knowledge_representation.py:176-211 -> KGStepper) through the C ABI and, in a single process, replayed from one HIP graph per
step kind.  Where a one-launch step kernel exists (ktup_train_step_supported: TUP / KTUP at d in {64, 100, 128}, TransH / TransE at
any d % 4 == 0; ktup_train_transr_step; ktup_train_transd_step) a step is that launch -- scores, loss, regularisers, every gradient --
and ktup_optim_clip_step (norm, clip, optimizer, zero-fill of the gradients): TWO launches, FIVE for TUP, whose three row
regularisers are launches of their own between the two.  Otherwise (and with KTUP_FUSED_STEP=0) the round-1 sequence of about a
dozen launches runs: same arithmetic, separate kernels.  The argument lists of the launches that more than one stepper binds are
written once, in utils/step_plans.py; when a step is issued, captured or replayed is decided in one place, `_StepperBase._run`.

The autograd route (`model(...)`, `bprLoss`, `.backward()`, `clip_and_step`) costs ~50 launches and ~0.5 ms of Python per
B=512 step: every Function allocates and zero-fills table-shaped gradients which autograd then adds into `.grad`, and
positives and negatives are scored by separate launches.  Here positives and negatives share one forward and one
backward launch (ids concatenated in fixed buffers), the backward kernels accumulate straight into the persistent,
zero-filled `.grad` tensors, and the optimizer pass leaves them zeroed for the next step.  Same kernels, same
arithmetic: tests/test_fast_train.py checks the tables against the autograd route after a mixed rec/kg schedule.

Data parallel (config 4, torchrun, one process per GPU): every rank keeps all tables, takes rows [rank*B/G, (rank+1)*B/G)
of the step's global batch, and ONE all-reduce (RCCL) of a flat bucket -- all gradients are views into it, the loss
scalars ride at its end -- precedes the clip + step, which is then identical on every rank.  Loss terms scale as in
jTransUP/parallel.py: batch means and whole-table regularisers by 1/G, batch sums unchanged.

rec step (knowledgable_recommendation.py:335-344):  bprLoss(pos, neg, target=-1) + orthogonalLoss(pref, pref_norm)
kg step  (:345-382):  kg_lambda * ( marginLoss(pos, neg, margin) + orthogonalLoss(rel, norm)[rel ids]
                                    + normLoss(ent)[h, t ids of pos and neg] + normLoss(rel)[rel ids] )
"""
import os

import torch
import torch.distributed as dist

from jTransUP.hip import lib as L
from jTransUP.hip import ops
from jTransUP.utils import step_plans as plans
from jTransUP.utils.step_plans import _p


class _StepperBase(object):
    """Shared machinery: flat gradient bucket (grads are views, 8 loss scalars at its end), data-parallel slice + all-reduce,
    pre-bound launches, HIP-graph replay, the K20 clip + step.  A subclass gives `_setup`, `_bind` (the launch plans) and
    `_rec_launches` / `_kg_launches` (a step's launches on bound plans and packed ids; they return the step's loss tensor)."""

    KINDS = ()        # step kinds of the subclass, e.g. ('rec', 'kg'), with the number of id tensors each takes
    N_IDS = {}
    READOPT_GRADS = True      # the all-reduce hands a parameter whose `.grad` left the flat bucket its view back (False: a subclass keeps some at None)

    def __init__(self, model, trainer, FLAGS, batch_size, group=None, use_graphs=None):
        if trainer.fused is None:
            raise L.KtupError('the GPU-resident step needs the fused optimizer (KTUP_FUSED_OPTIM=0 disables it)')
        self.m, self.trainer = model, trainer
        self.group = group
        self.world = dist.get_world_size(group) if dist.is_initialized() else 1
        self.rank = dist.get_rank(group) if dist.is_initialized() else 0
        if int(batch_size) % self.world:
            raise L.KtupError('batch_size %d is not divisible by the %d data-parallel ranks' % (batch_size, self.world))
        self.GB = int(batch_size)                    # global batch (what the driver samples)
        self.B = self.GB // self.world               # rows this rank scores
        self.margin, self.max_norm = float(FLAGS.margin), float(FLAGS.clipping_max_value)
        self.target = float(trainer.model_target)
        self.l1 = int(bool(getattr(model, 'L1_flag', False)))
        self.tabs = tuple(trainer.parameters)
        dev = self.tabs[0].device
        self.dev = dev
        f32 = dict(dtype=torch.float32, device=dev)
        i64 = dict(dtype=torch.int64, device=dev)
        # persistent zero-filled gradients (torch 0.3 zero_grad semantics) as views into one flat bucket with 8 loss scalars at
        # its end: parallel.ReplicaGradSync owns the bucket and its ONE all-reduce per step
        from jTransUP.parallel import ReplicaGradSync
        self.sync = ReplicaGradSync(trainer.parameters, group=group, extra=8)
        self.flat, self.loss = self.sync.flat, self.sync.extra
        if self.world > 1:                           # identical replicas to start from
            for p in trainer.parameters:
                dist.broadcast(p.data, src=0, group=group)
        B = self.B
        self.score, self.gscore = torch.zeros(2 * B, **f32), torch.zeros(2 * B, **f32)
        self.inv_world = torch.full((), 1.0 / self.world, **f32)                         # upstream gradient of 'mean' / 'replicated' terms
        self.one = torch.ones((), **f32)
        self._keys = None
        self._stream = None
        # HIP graphs: with a step-independent optimizer every launch argument of a step is static (the ST-Gumbel stream
        # position lives in device memory, KTUP_GUMBEL_PHILOX_DEV), so the launches of a step replay as ONE graph launch
        # (KTUP_TRAIN_GRAPHS=0 disables).  Inputs are copied into fixed buffers first.
        if use_graphs is None:
            use_graphs = os.environ.get('KTUP_TRAIN_GRAPHS', '1') != '0'
        # Data-parallel replicas: the step is still ONE graph -- fused step kernel, the all-reduce of the flat bucket (RCCL
        # collectives are capturable), clip + optimizer launch -- when the backend is nccl; under the gloo test hook the
        # all-reduce is staged through the host and the launches are issued one by one (KTUP_DP_GRAPHS=0 forces that too)
        # Several ranks: capturing the all-reduce inside the step's graph is exercised over RCCL at world 1 only (this repo's boxes
        # have one GPU), so it is opt-in there (KTUP_DP_GRAPHS=1) and the default issues the launches and the collective one by
        # one; every rank takes the same route (same environment, same step counts).
        dp_ok = self.world == 1 or (dist.get_backend(group) == 'nccl' and os.environ.get('KTUP_DP_GRAPHS', '0') == '1')
        if dist.is_initialized() and self.world == 1 and dist.get_backend(group) != 'nccl':
            from jTransUP import parallel as _par
            dp_ok = not _par._FORCE[0]              # forced collectives on gloo stage through the host: not capturable
        self.use_graphs = bool(use_graphs) and dp_ok
        self.never_captured = frozenset()           # step kinds whose launches are always issued one by one (a subclass says why)
        self.want_fused = os.environ.get('KTUP_FUSED_STEP', '1') != '0'
        self.out = {k: torch.zeros((), **f32) for k in self.KINDS}                       # fused steps: where the step's loss is published
        # the gradient norm without a pass over the gradients (include/ktup_hip.h `gnorm`): the fused step kernels track the squared
        # norm of the buffers their atomics build, ktup_optim_clip_step reads it -- one process only (an all-reduce of the gradients
        # changes their norm), only with clipping on, and for d <= 128 (at d = 256 the rec step kernel has no registers left for the
        # returned values).  KTUP_TRACKED_NORM=0: the norm pass + grid barrier of round 2.
        self._gn = None
        # (FM's and coFM's first parameter is their global bias, one element: their steps track no norm)
        if self.world == 1 and self.max_norm > 0 and self.tabs[0].dim() == 2 and self.tabs[0].shape[1] <= 128 \
                and os.environ.get('KTUP_TRACKED_NORM', '1') != '0':
            self._gn = torch.zeros(64, dtype=torch.float64, device=dev)                 # KTUP_GNORM_WS_DOUBLES
        self._graphs = {}
        self._eager_steps = {k: 0 for k in self.KINDS}
        self.replays = {k: 0 for k in self.KINDS}                                        # host-fed steps that were replays of the step's graph
        self.fed_replays = {k: 0 for k in self.KINDS}                                    # device-fed steps that were (part of) a graph replay
        self._feeds, self._sampler, self._feed_launch, self._feed_ok = {}, None, {}, {}
        self._acc_on = False
        self.acc = {k: torch.zeros((), **f32) for k in self.KINDS}                       # fed steps: running sum of the steps' losses
        self.gstate = self.guni = None              # the hard preference gate: device stream position (_gumbel_stream), parity uniforms
        self._setup(FLAGS, f32, i64)

    # ------------------------------------------------------------------------------------------------ device-fed steps
    def attach_feeds(self, sampler, **feeds):
        """-device_sampling: `feeds[kind]` (DeviceFeeder) + `sampler` (DeviceSampler) let a step of that kind build its own batch
        on the device (ktup_feed_rec / ktup_feed_kg, captured in the step's graph): `fed_step(kind)` then needs no id tensors
        and no host work besides the graph replay.  Single process only (replicas slice one global batch per step)."""
        self._sampler = sampler
        self._feeds = dict(feeds)
        self._feed_ok = {}
        self._keys = None                       # bind the feed launches with the next plan

    def can_feed(self, kind):
        ok = self._feed_ok.get(kind)
        if ok is None:
            ok = False
            if kind in self._feeds and self.world == 1:
                self._plans()                   # decides fused_step for this shape
                ok = bool(self._feedable())     # the multi-launch routes take id arrays the feed launches do not fill
            self._feed_ok[kind] = ok
        return ok

    def _feedable(self):
        """Does the bound step read nothing but the [pos ; neg] id arrays the feed launches fill?"""
        return self.fused_step

    def _acc_ptr(self, kind):
        """Fed steps: the optimizer launch adds the step's loss to acc[kind] itself."""
        return _p(self.acc[kind]) if self._acc_on else None

    def _make_feed(self, kind, st):
        b, sm, feed = L.bind, self._sampler, self._feeds[kind]
        if kind == 'rec':
            return b('ktup_feed_rec', _p(feed.cols[0]), _p(feed.cols[1]), feed.n, self.B, _p(feed.cursor), _p(sm.offset_dev[0:]),
                     sm.n_items, _p(sm.bitmap), sm.words if sm.bitmap is not None else 0, sm.seed, 1, _p(self.u2), _p(self.i2),
                     _p(sm.rec_workspace()), _p(sm.fail), st)
        return b('ktup_feed_kg', _p(feed.cols[0]), _p(feed.cols[1]), _p(feed.cols[2]), feed.n, self.B, _p(feed.cursor),
                 _p(sm.offset_dev[1:]), sm.n_ent, sm.n_rel, _p(sm.keys), 0 if sm.keys is None else sm.keys.numel(), sm.seed,
                 _p(self.h2), _p(self.t2), _p(self.r2), _p(sm.fail), st)

    def _bind_feeds(self, st):
        self._feed_launch = {kind: self._make_feed(kind, st) for kind in self._feeds}

    def take_sums(self):
        """{kind: sum of the losses of the fed steps since the last call} (one sync; the fed steps accumulate on the device)."""
        out = {k: float(v.item()) for k, v in self.acc.items()}
        for v in self.acc.values():
            v.zero_()
        return out

    def _gumbel_stream(self, draws_per_step):
        """The device-side stream position of the hard preference gate: uint64[2] = {seed, offset}; `_gumbel_advance()` moves the
        offset past a step's draws (a captured launch).  Without the gate `gstate` stays None."""
        if not getattr(self.m, 'use_st_gumbel', False):
            return
        seed = (int(self.m._gumbel.seed) * 6364136223846793005 + 1442695040888963407) % (1 << 62)   # own stream, apart from eval's
        self.gstate = torch.tensor([seed, 0], dtype=torch.int64, device=self.dev)
        self.gadv = torch.tensor([0, int(draws_per_step)], dtype=torch.int64, device=self.dev)

    def _gate_args(self):
        """(mode, pointer argument) of the preference gate."""
        if self.gstate is not None and self.guni is not None:
            return (ops.GUMBEL_INPUT, _p(self.guni))
        return (ops.GUMBEL_OFF, None) if self.gstate is None else (ops.GUMBEL_PHILOX_DEV, _p(self.gstate))

    def set_gumbel_uniforms(self, uniforms):
        """Parity hook (tests against the reference's goldens): the ST-Gumbel gate of the NEXT steps reads its uniforms -- one row
        of n_pref values per scored pair, positives then negatives, as transUP.py:159-162 drew them -- from a fixed buffer that
        this call fills, instead of drawing Philox numbers on the device.  None switches back."""
        if self.gstate is None:
            raise L.KtupError('the model has no ST-Gumbel gate')
        if uniforms is None:
            if self.guni is not None:                  # bound launches and captured graphs still point at the uniform buffer
                self._keys = None
                self._graphs = {}
                self._eager_steps = {k: 0 for k in self.KINDS}
            self.guni = None
        else:
            if self.guni is None:
                self.guni = torch.empty(2 * self.B, uniforms.shape[1], dtype=torch.float32, device=self.dev)
                self._keys = None                      # re-bind the launches with the new gate arguments
                self._graphs = {}
            self.guni.copy_(uniforms)

    def _gumbel_advance(self):
        if self.gstate is not None:
            self.gstate.add_(self.gadv)

    def _mine(self, t):
        """This rank's rows of a global-batch id tensor."""
        return t if self.world == 1 else t[self.rank * self.B:(self.rank + 1) * self.B]

    def _id_buffers(self, kind, i64):
        """The persistent [pos ; neg] id arrays of a step kind as views of ONE buffer, so that `_pack` fills them with one
        torch.cat (one launch and one dispatch per step instead of two for a rec step, four for a kg step)."""
        B = self.B
        if kind == 'rec':
            self._ids_rec = torch.zeros(4 * B, **i64)
            self.u2, self.i2 = self.rec_ids = self._ids_rec[:2 * B], self._ids_rec[2 * B:]     # [u ; u], [pos ; neg]
        else:
            self._ids_kg = torch.zeros(10 * B, **i64)
            self.h2, self.t2, self.r2 = self._ids_kg[:2 * B], self._ids_kg[2 * B:4 * B], self._ids_kg[4 * B:6 * B]
            self.ht4 = self._ids_kg[6 * B:]                                              # ph, pt, nh, nt (normLoss rows)
            self.kg_ids = (self.h2, self.t2, self.r2, self.ht4)

    def _pack(self, kind, args):
        if kind == 'rec':
            u, pi, ni = (self._mine(x) for x in args)
            torch.cat((u, u, pi, ni), out=self._ids_rec)
        else:
            ph, pt, pr, nh, nt, nr = (self._mine(x) for x in args)
            torch.cat((ph, nh, pt, nt, pr, nr, ph, pt, nh, nt), out=self._ids_kg)

    def _g(self, t):
        """Pointer of table t's gradient buffer (what the launch plans write into and `_plans` keys on)."""
        return t.grad.data_ptr()

    def _plans(self):
        """Every launch of a step has fixed arguments (persistent buffers): marshal them once (lib.bind).  Re-done when a table's
        or a gradient's storage moves (load_state_dict keeps storages, so in practice never) or the stream changes (graph capture)."""
        st = torch.cuda.current_stream(self.dev).cuda_stream
        keys = tuple(t.data_ptr() for t in self.tabs) + tuple(self._g(t) for t in self.tabs)
        if self._keys != keys or st != self._stream:
            self._keys, self._stream = keys, st
            self._bind(st)
            if self._feeds:
                self._bind_feeds(st)

    def _gn_ptr(self):
        return None if self._gn is None else _p(self._gn)

    def _optimizer_launches(self, loss=None, tracked=False):
        """`tracked`: the launch before this one was a fused step bound with the gradient-norm workspace."""
        self.sync.all_reduce_grads(readopt=self.READOPT_GRADS)   # world > 1: gradients of all tables + the loss scalars, one bucket, one collective
        self.trainer.fused.clip_and_step(self.max_norm, zero_grads=True, loss=loss, gnorm=self._gn_ptr() if tracked else None)

    def _fused_ok(self, kind, d, n_pref=0):
        ok = bool(self.want_fused and L.load().ktup_train_step_supported(kind, d, n_pref))
        if not ok and L.get_option('deterministic'):
            # KTUP_DETERMINISTIC=1 (include/ktup_hip.h option "deterministic"): only the fused step kernels have the one-workgroup
            # form whose gradient sums do not depend on the order atomics land in; the multi-launch route would silently not have it
            raise L.KtupError('KTUP_DETERMINISTIC=1 needs a fused step kernel; this shape (kind %d, d=%d, n_pref=%d) has none' % (kind, d, n_pref))
        return ok

    # ------------------------------------------------------------------------------------------------ issue, capture, replay
    def _launches(self, kind, ids, fed):
        """One step's launches on the current stream: the feed launch (fed) or the id pack (host-fed; ids None: already packed),
        then the kind's own launches.  Returns the step's loss tensor."""
        self._plans()
        if fed:
            self._feed_launch[kind]()
        elif ids is not None:
            self._pack(kind, ids)                                # ids -> the persistent [pos ; neg] buffers
        self._acc_on = fed
        try:
            return self._rec_launches() if kind == 'rec' else self._kg_launches()
        finally:
            self._acc_on = False

    def _run(self, gkey, kinds, ids=None, fed=False, cycle=False):
        """The steps `kinds` -- ONE step (`_step`, `fed_step`) or a cycle of device-fed steps (`fed_cycle`) -- issued launch by
        launch, or captured into / replayed from the graph `_graphs[gkey]` = (graph, output tensor, the optimizer it was captured
        with).  Host-fed steps bring `ids`; fed steps draw their batches on the device.  The rules, all of them:

        - Eager route: when `use_graphs` is off, `fused.graph_safe()` is false or a kind is in `never_captured`.  A cycle returns 0.
        - An entry whose third element is not the trainer's current `fused` (the trainer re-created its optimizer: LR decay) is
          dropped.  For a single step this also resets the kind's warm-up counter; a cycle does not reset it.
        - A cycle returns 0 -- before any host accounting -- whenever a kind's '+fed' entry is missing or stale (warm-up, lazy
          optimizer state) or a feeder's epoch would end inside the cycle (the host reshuffles between replays, never inside one).
        - Two eager warm-up steps per kind (allocations, lazy optimizer state) come before its first capture, counted in ONE
          counter that `kind` and `kind + '+fed'` share.
        - Host-fed steps pack their ids (`_pack`) before the capture or the replay, outside the graph; the captured body gets None.
        - Fed steps call `feed.fed()` and `sampler.fed(B, kind)` before anything else, the eager route included.
        - `_acc_on` is true only around a fed body (`_launches`).
        - After a capture `_keys = None` and `fused._plan = None`: both were bound to the capture stream.
        - `bump_steps(n)` and the `replays` / `fed_replays` counters advance on replays only: the capturing pass already ran the
          host side of clip_and_step (its graph is launched once too).
        - `trainer.step` advances by the number of steps in every case.
        Returns the step's loss tensor (for a graph: the captured output, entry[1]), or the step count for a cycle."""
        fused, kind, n = self.trainer.fused, kinds[0], len(kinds)
        graphs = self.use_graphs and fused.graph_safe() and self.never_captured.isdisjoint(kinds)
        if cycle:
            if not graphs:
                return 0
            count = {}
            for k in kinds:
                count[k] = count.get(k, 0) + 1
            for k, c in count.items():
                entry, feed = self._graphs.get(k + '+fed'), self._feeds.get(k)
                if entry is None or entry[2] is not fused or feed.start + (c - 1) * self.B > feed.n - self.B:
                    return 0
        if fed:
            for k in kinds:
                self._feeds[k].fed()
                self._sampler.fed(self.B, k)
        entry = self._graphs.get(gkey) if graphs else None
        if entry is not None and entry[2] is not fused:
            entry = None
            if not cycle:
                self._eager_steps[kind] = 0
        if not graphs or (entry is None and not cycle and self._eager_steps[kind] < 2):
            if graphs:
                self._eager_steps[kind] += 1
            out = self._launches(kind, ids, fed)
            self.trainer.step += 1
            return out
        if not fed:
            self._pack(kind, ids)
        if entry is None:
            graph = torch.cuda.CUDAGraph()
            with L.capture(graph):
                for k in kinds:
                    out = self._launches(k, None, fed)
            self._keys = None
            fused._plan = None
            entry = self._graphs[gkey] = (graph, None if cycle else out, fused)
            graph.replay()
        else:
            entry[0].replay()
            fused.bump_steps(n)
            counter = self.fed_replays if fed else self.replays
            for k in kinds:
                counter[k] += 1
        self.trainer.step += n
        return n if cycle else entry[1]

    def _step(self, kind, ids):
        return self._run(kind, (kind,), ids)

    def fed_step(self, kind):
        """One step of `kind` on the feeder's next batch: the step's graph is  feed launch -> step kernel -> clip + optimizer
        launch, and the host does nothing but replay it.  The optimizer launch adds the step's loss to `acc[kind]` (take_sums).
        (Drawing the NEXT batch on a side stream beside the optimizer launch was built and measured: the fork / join inside the
        graph costs more than the 8 us it hides -- 56 vs 50 us per step.)"""
        return self._run(kind + '+fed', (kind,), fed=True)

    def fed_cycle(self, kinds):
        """len(kinds) consecutive fed steps as ONE graph replay (hipGraphLaunch + the Python around it cost ~5 us per replay --
        a tenth of a step).  Returns len(kinds), or 0 when the cycle cannot run right now (`_run`)."""
        return self._run('cycle:' + ','.join(kinds), kinds, fed=True, cycle=True)

    # ------------------------------------------------------------------------------------------------ public steps
    def rec_step(self, u, pi, ni):
        """u, pi, ni: int64 device tensors of the GLOBAL batch.  Returns the step's loss (0-dim device tensor)."""
        return self._step('rec', (u, pi, ni))

    def kg_step(self, ph, pt, pr, nh, nt, nr):
        return self._step('kg', (ph, pt, pr, nh, nt, nr))


class JointStepper(_StepperBase):
    """KTUP (jtransup, own tables): knowledgable_recommendation.py:330-401."""
    KINDS = ('rec', 'kg')
    N_IDS = {'rec': 3, 'kg': 6}

    def _setup(self, FLAGS, f32, i64):
        model, B = self.m, self.B
        self.kg_lambda = float(FLAGS.kg_lambda)
        U, I, E, P, Pn, R, Rn = model._rec_tables()
        self.tabs = (U, I, E, P, Pn, R, Rn)
        self._id_buffers('rec', i64); self._id_buffers('kg', i64)
        self.gAC = torch.zeros(2, P.shape[0], P.shape[1], **f32)                         # mixed-table gradients gA, gC
        self.lam = torch.full((), self.kg_lambda, **f32)                                 # upstream gradient of the KG 'sum' terms
        self.ws = ops.pref_workspace(P, Pn, R, Rn)
        self.ent_pad = model.ent_total - 1
        self.i2e = model._item2ent
        self._gumbel_stream(2 * B * P.shape[0])

    # ------------------------------------------------------------------------------------------------ launch plans
    def _bind(self, st):
        U, I, E, P, Pn, R, Rn = self.tabs
        B, b, g = self.B, L.bind, self._g
        n_pref, d = P.shape
        pos, neg, gpos, gneg = self.score[:B], self.score[B:], self.gscore[:B], self.gscore[B:]
        gate, gptr = self._gate_args()
        self.fused_step = self._fused_ok(0, d, n_pref) and self._fused_ok(1, d)
        if self.fused_step:
            self._rec_fused = plans.rec_step(U, I, P, Pn, self.rec_ids, B, self.l1, (gate, gptr), self.target, 1.0 / self.world, self.loss,
                                             g, self._gn_ptr(), st, E=E, i2e=self.i2e, ent_pad=self.ent_pad, R=R, Rn=Rn)
            self._kg_fused = plans.kg_step(E, R, Rn, self.kg_ids, B, self.l1, self.margin, self.kg_lambda, self.loss, g, self._gn_ptr(), st)
        self._rec_head = [
            b('ktup_pref_prepare', _p(P), _p(Pn), _p(R), _p(Rn), P.stride(0), n_pref, d, _p(self.ws), st)]
        self._rec_soft = [
            b('ktup_score_ktup_fwd', _p(U), U.stride(0), _p(I), I.stride(0), _p(E), E.stride(0), _p(self.i2e), _p(self.ws), n_pref, d,
              _p(self.u2), _p(self.i2), 2 * B, self.l1, gate, gptr, 0, 0, _p(self.score), st)]
        # value + gradient in one launch; the loss slots are zeroed once at the top of a step and accumulated into
        self._rec_loss = [
            b('ktup_loss_bpr_fused', _p(pos), _p(neg), B, self.target, _p(self.inv_world), _p(self.loss[0:]), _p(gpos), _p(gneg), st)]
        self._rec_soft_bwd = [
            b('ktup_score_ktup_bwd', _p(U), U.stride(0), _p(I), I.stride(0), _p(E), E.stride(0), _p(self.i2e), self.ent_pad,
              _p(self.ws), n_pref, d, _p(self.u2), _p(self.i2), 2 * B, self.l1, gate, gptr, 0, 0,
              _p(self.gscore), _p(U.grad), _p(I.grad), _p(E.grad), _p(self.gAC[0]), _p(self.gAC[1]), st)]
        self._rec_tail = [
            b('ktup_reg_orth_fused', _p(P), P.stride(0), _p(Pn), Pn.stride(0), d, None, n_pref, _p(self.inv_world), _p(self.loss[1:]),
              _p(P.grad), _p(Pn.grad), st)]
        self._kg = plans.kg_sequence('transh', (E, R, Rn), self.kg_ids, B, self.l1, self.margin, self.score, self.gscore, self.loss,
                                     self.lam, g, st)

    # ------------------------------------------------------------------------------------------------ rec
    def _rec_launches(self):
        if self.fused_step:              # one launch: table mixing, both scores, bprLoss, backward, gradient fan-out, orthogonalLoss
            self._rec_fused()
            self._gumbel_advance()
            if self.world > 1:
                self.loss[:2].mul_(self.inv_world)
            self._optimizer_launches(loss=(_p(self.loss), 2, 1.0, _p(self.out['rec']), self._acc_ptr('rec')), tracked=True)
            return self.out['rec']
        U, I, E, P, Pn, R, Rn = self.tabs
        self._rec_head[0]()
        self.gAC.zero_(); self.loss.zero_()
        self._rec_soft[0](); self._rec_loss[0](); self._rec_soft_bwd[0]()
        self._gumbel_advance()
        # A = pref + rel and C = pref_norm + norm: the mixed-table gradient goes to both summands
        torch._foreach_add_([P.grad, R.grad, Pn.grad, Rn.grad], [self.gAC[0], self.gAC[0], self.gAC[1], self.gAC[1]])
        self._rec_tail[0]()
        if self.world > 1:
            self.loss[:2].mul_(self.inv_world)
        self._optimizer_launches()
        return self.loss[0] + self.loss[1]

    # ------------------------------------------------------------------------------------------------ kg
    def _kg_launches(self):
        if self.fused_step:              # one launch: both TransH scores, marginLoss, the three regularisers, every gradient
            self._kg_fused()
            self._optimizer_launches(loss=(_p(self.loss), 4, self.kg_lambda, _p(self.out['kg']), self._acc_ptr('kg')), tracked=True)
            return self.out['kg']
        self.loss.zero_()
        for launch in self._kg:
            launch()
        self._optimizer_launches()
        return self.kg_lambda * self.loss[:4].sum()


class RecStepper(_StepperBase):
    """Rec-only driver (item_recommendation.py:160-195): TUP (transup) with its regularisers (:177-180), or BPRMF (bpr only).
    loss slots: 0 bpr, 1 orthogonalLoss(pref, pref_norm), 2 normLoss(user rows), 3 normLoss(item rows), 4 normLoss(pref)."""
    KINDS = ('rec',)
    N_IDS = {'rec': 3}

    def _setup(self, FLAGS, f32, i64):
        model, B = self.m, self.B
        self.tup = hasattr(model, 'pref_embeddings')
        if self.tup:
            U, I, P, Pn = model._tables()
            self.tabs = (U, I, P, Pn)
            self.gAC = torch.zeros(2, P.shape[0], P.shape[1], **f32)
            self.ws = ops.pref_workspace(P, Pn)
        else:
            self.tabs = (model.user_embeddings.weight, model.item_embeddings.weight)
        self._id_buffers('rec', i64)
        self._gumbel_stream(2 * B * self.tabs[2].shape[0] if self.tup else 0)

    def _bind(self, st):
        B, b = self.B, L.bind
        U, I = self.tabs[0], self.tabs[1]
        d = U.shape[1]
        pos, neg, gpos, gneg = self.score[:B], self.score[B:], self.gscore[:B], self.gscore[B:]
        self._loss = [b('ktup_loss_bpr_fused', _p(pos), _p(neg), B, self.target, _p(self.inv_world), _p(self.loss[0:]), _p(gpos),
                        _p(gneg), st)]
        self.fused_step = False
        if not self.tup:
            self._fused_ok(-1, d)                          # (raises under KTUP_DETERMINISTIC=1: BPRMF steps are several launches with plain atomics)
            self._fwd = b('ktup_score_bprmf_fwd', _p(U), U.stride(0), _p(I), I.stride(0), d, _p(self.u2), _p(self.i2), 2 * B,
                          _p(self.score), st)
            self._bwd = b('ktup_score_bprmf_bwd', _p(U), U.stride(0), _p(I), I.stride(0), d, _p(self.u2), _p(self.i2), 2 * B,
                          _p(self.gscore), _p(U.grad), _p(I.grad), st)
            return
        P, Pn = self.tabs[2], self.tabs[3]
        n_pref = P.shape[0]
        gate, gptr = self._gate_args()
        self.fused_step = self._fused_ok(0, d, n_pref)
        if self.fused_step:              # (no tracked norm: the row regularisers below add to the gradients after this launch)
            self._rec_fused = plans.rec_step(U, I, P, Pn, self.rec_ids, B, self.l1, (gate, gptr), self.target, 1.0 / self.world, self.loss,
                                             self._g, None, st)
        self._prep = b('ktup_pref_prepare', _p(P), _p(Pn), None, None, P.stride(0), n_pref, d, _p(self.ws), st)
        self._fwd = b('ktup_score_tup_fwd', _p(U), U.stride(0), _p(I), I.stride(0), _p(self.ws), n_pref, d, _p(self.u2), _p(self.i2),
                      2 * B, self.l1, gate, gptr, 0, 0, _p(self.score), st)
        self._bwd = b('ktup_score_tup_bwd', _p(U), U.stride(0), _p(I), I.stride(0), _p(self.ws), n_pref, d, _p(self.u2), _p(self.i2),
                      2 * B, self.l1, gate, gptr, 0, 0, _p(self.gscore), _p(U.grad), _p(I.grad), _p(self.gAC[0]), _p(self.gAC[1]), st)
        self._regs = [
            b('ktup_reg_orth_fused', _p(P), P.stride(0), _p(Pn), Pn.stride(0), d, None, n_pref, _p(self.inv_world), _p(self.loss[1:]),
              _p(P.grad), _p(Pn.grad), st),
            b('ktup_reg_norm_fused', _p(U), U.stride(0), d, _p(self.u2), B, _p(self.one), _p(self.loss[2:]), _p(U.grad), st),      # the step's users once
            b('ktup_reg_norm_fused', _p(I), I.stride(0), d, _p(self.i2), 2 * B, _p(self.one), _p(self.loss[3:]), _p(I.grad), st),  # pos and neg items
            b('ktup_reg_norm_fused', _p(P), P.stride(0), d, None, n_pref, _p(self.inv_world), _p(self.loss[4:]), _p(P.grad), st)]

    def _rec_launches(self):
        self.loss.zero_()
        if not self.tup:
            self._fwd(); self._loss[0](); self._bwd()
            if self.world > 1:
                self.loss[:1].mul_(self.inv_world)
            self._optimizer_launches()
            return self.loss[0] + 0.0
        U, I, P, Pn = self.tabs
        if self.fused_step:              # scores, bprLoss, backward and orthogonalLoss in one launch; the row regularisers follow
            self._rec_fused()
            self._gumbel_advance()
            for launch in self._regs[1:]:
                launch()
            if self.world > 1:
                self.loss[:2].mul_(self.inv_world); self.loss[4:5].mul_(self.inv_world)
            self._optimizer_launches(loss=(_p(self.loss), 5, 1.0, _p(self.out['rec']), self._acc_ptr('rec')))
            return self.out['rec']
        self._prep()
        self.gAC.zero_()
        self._fwd(); self._loss[0](); self._bwd()
        self._gumbel_advance()
        torch._foreach_add_([P.grad, Pn.grad], [self.gAC[0], self.gAC[1]])
        for launch in self._regs:
            launch()
        if self.world > 1:       # batch mean and whole-table terms by 1/G, batch sums as they are
            self.loss[:2].mul_(self.inv_world); self.loss[4:5].mul_(self.inv_world)
        self._optimizer_launches()
        return self.loss[:5].sum()


class KGStepper(_StepperBase):
    """KG-only driver (knowledge_representation.py:176-211) for TransE / TransH / TransR / TransD: marginLoss + normLoss(entity rows
    of the positive and negative triples) + normLoss(relation rows) (+ orthogonalLoss(rel, norm) rows for TransH).  TransD's two
    projection tables take the score gradient only (no regulariser touches them, knowledge_representation.py:200-204)."""
    KINDS = ('kg',)
    N_IDS = {'kg': 6}

    def _setup(self, FLAGS, f32, i64):
        model, B = self.m, self.B
        self.transh = hasattr(model, 'norm_embeddings')
        self.transr = hasattr(model, 'proj_embeddings')
        self.transd = hasattr(model, 'ent_proj_embeddings')
        self.model_kind = 'transh' if self.transh else 'transr' if self.transr else 'transd' if self.transd else 'transe'
        E, R = model.ent_embeddings.weight, model.rel_embeddings.weight
        self.tabs = (E, R, model.norm_embeddings.weight) if self.transh else (E, R, model.proj_embeddings.weight) if self.transr else (E, R)
        if self.transd:
            self.tabs = (E, R, model.ent_proj_embeddings.weight, model.rel_proj_embeddings.weight)
        # TransR: the whole step as ONE launch (ktup_train_transr_step; KTUP_FUSED_STEP=0 keeps the bucketed multi-launch route).
        # `fused_step` stays False for it: the device-fed steps are not built for TransR, which takes its batches from the host.
        self.transr_step = bool(self.transr and self.want_fused and L.load().ktup_train_transr_step_supported(E.shape[1])
                                and 1 <= B <= 4096 and 1 <= min(R.shape[0], self.tabs[2].shape[0]) <= 4096)
        # The bucketed TransR kernels (d = 64, 100, 128) clear their counters with a memset into a pooled workspace; a captured
        # memset node of that kind writes garbage from its second replay on, so that route is never captured:
        # it is issued launch by launch, as BaselineJointStepper's kg step is for CKE.
        if self.transr and not self.transr_step and E.shape[1] in (64, 100, 128):
            self.never_captured = frozenset(['kg'])
        # TransD: the whole step as ONE launch too (ktup_train_transd_step; KTUP_FUSED_STEP=0 keeps the multi-launch route).  It reads
        # the [pos ; neg] id arrays alone, so the device-fed steps take it (`_feedable`); `fused_step` stays False for it as well.
        self.transd_step = bool(self.transd and self.want_fused and L.load().ktup_train_transd_step_supported(E.shape[1])
                                and all(t.data_ptr() % 16 == 0 and t.stride(0) % 4 == 0 and t.stride(1) == 1 and t.grad is not None
                                        and t.grad.data_ptr() % 16 == 0 and t.grad.stride() == t.stride() for t in self.tabs))
        self.rws = None
        if self.transr and not self.transr_step:             # scratch of the relation-bucketed forward (K4)
            nbytes = L.load().ktup_score_transr_workspace_bytes(2 * B, R.shape[0])
            self.rws = torch.empty((nbytes + 3) // 4, dtype=torch.int32, device=self.dev)
        self._id_buffers('kg', i64)

    def _bind(self, st):
        E, R = self.tabs[0], self.tabs[1]
        d = E.shape[1]
        step = (self.kg_ids, self.B, self.l1, self.margin, 1.0, self.loss, self._g)       # what the one-launch builders share
        # (-1: no kernel of ktup_train_step_supported; TransR's and TransD's one-launch steps are `transr_step` / `transd_step`.  TransD's
        # has the one-workgroup form of option `deterministic`, so it is not refused under KTUP_DETERMINISTIC=1.)
        self.fused_step = False if self.transd_step else \
            self._fused_ok(-1 if (self.transr or self.transd) else (1 if self.transh else 2), d)
        self._calls = []
        if self.transd_step:
            self._transd_fused = plans.transd_step(E, R, self.tabs[2], self.tabs[3], *step, self._gn_ptr(), st)
            return
        if self.fused_step:
            self._kg_fused = plans.kg_step(E, R, self.tabs[2] if self.transh else None, *step, self._gn_ptr(), st)
        if self.transr_step:
            self._transr_fused = plans.transr_step(E, R, self.tabs[2], *step, st)
            return
        self._calls = plans.kg_sequence(self.model_kind, self.tabs, self.kg_ids, self.B, self.l1, self.margin, self.score, self.gscore,
                                        self.loss, self.one, self._g, st, rws=self.rws)

    def _kg_launches(self):
        if self.fused_step:
            self._kg_fused()
            self._optimizer_launches(loss=(_p(self.loss), 4, 1.0, _p(self.out['kg']), self._acc_ptr('kg')), tracked=True)
            return self.out['kg']
        if self.transr_step:             # one launch: both TransR scores, marginLoss, the two regularisers, every gradient
            self._transr_fused()
            self._optimizer_launches(loss=(_p(self.loss), 4, 1.0, _p(self.out['kg']), self._acc_ptr('kg')))
            return self.out['kg']
        if self.transd_step:             # one launch: both TransD scores, marginLoss, the two regularisers, the gradients of all four tables
            self._transd_fused()
            self._optimizer_launches(loss=(_p(self.loss), 4, 1.0, _p(self.out['kg']), self._acc_ptr('kg')), tracked=self._gn is not None)
            return self.out['kg']
        self.loss.zero_()
        for launch in self._calls:
            launch()
        self._optimizer_launches()
        return self.loss[:4].sum()

    def _feedable(self):
        return self.fused_step or self.transd_step


class DeviceFeeder(object):
    """Device-resident training data for the GPU-resident loop: the rating / triple lists as device tensors, an epoch
    permutation drawn on the device, batches as slices, negatives from the K19 samplers (utils/device_sampler.py).
    Iterator contract of utils/data.py MakeTrainIterator (data.py:87-110): endless, the order list holds `negtive_samples`
    copies of every example, and -- exactly like the reference -- it wraps (reshuffles) once `start > n - batch_size` with
    n = the number of DISTINCT examples, so only the first n entries of each shuffled order are consumed, and the tail
    partial batch is dropped.  -device_sampling and -nodevice_sampling therefore share one epoch / shuffle cadence."""

    def __init__(self, rows, batch_size, device, negtive_samples=1, seed=0):
        rows = torch.as_tensor(rows, dtype=torch.int64).reshape(len(rows), -1)[:, :3].to(device)
        self.B, self.dev, self.rep = int(batch_size), device, int(negtive_samples)
        self.gen = torch.Generator(device=device)
        self.gen.manual_seed(int(seed))
        self.n = rows.shape[0]
        if self.n < self.B:
            # the reference slices a batch out of the replicated order list even when n < B <= n * negtive_samples
            # (data.py:87-110); here an epoch's columns hold the n distinct examples only, so a full batch must fit in them
            raise ValueError('fewer distinct training examples (%d) than one batch (%d): lower -batch_size (negtive_samples does '
                             'not add rows to an epoch of the device-resident feeder)' % (self.n, self.B))
        # column-major: a batch is then a contiguous SLICE of this epoch's shuffled columns (no per-step gather launches), and
        # the columns live in fixed storage, reshuffled in place -- what the feed kernels' graph-static arguments point at
        self.src = [rows[:, c].contiguous() for c in range(rows.shape[1])]
        self.cols = [torch.empty(self.n, dtype=torch.int64, device=device) for _ in self.src]
        self.cursor = torch.zeros(1, dtype=torch.int64, device=device)      # device copy of `start` (ktup_feed_* advance it)
        self._shuffle()

    def _shuffle(self):
        self.order = order = (torch.randperm(self.n * self.rep, generator=self.gen, device=self.dev) % self.n)[:self.n]
        for src, col in zip(self.src, self.cols):
            torch.index_select(src, 0, order, out=col)
        self.start = 0
        self.cursor.zero_()
        self._cursor_ok = True

    def _take(self):
        if self.start > self.n - self.B:              # data.py:101-103: dataset_size, not len(order)
            self._shuffle()
        s = self.start
        self.start += self.B
        return s

    def next_cols(self):
        """The next batch as one contiguous 1-D view per column (no launches)."""
        s = self._take()
        self._cursor_ok = False
        return tuple(col[s:s + self.B] for col in self.cols)

    def next(self):
        return torch.stack(self.next_cols(), dim=1)

    def fed(self):
        """Account for one batch a ktup_feed_* launch is about to take (it moves the device cursor the same way)."""
        s = self._take()
        if not self._cursor_ok:
            self.cursor.fill_(s)
            self._cursor_ok = True
