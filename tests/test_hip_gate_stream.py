"""The hard (ST-Gumbel) gate's device noise, pinned to the documented stream in every kernel that walks it.

include/ktup_hip.h: in KTUP_GUMBEL_PHILOX / _PHILOX_DEV, row k of a call and preference p draw position offset + k * n_pref + p of
Philox4x32-10(seed) under the gate's tag.  So a Philox call must equal, score for score, the same call in KTUP_GUMBEL_INPUT fed
tests/philox_host.uniforms(seed, offset, n * P).reshape(n, P) -- forward AND backward: a backward that walks the stream one position
off, or drops the high half of the 64-bit block index, routes the gradient through another preference row than the forward scored with.

Which kernel a case reaches (read off run_pref in csrc/ktup_score_pref.hip, pref_fwd_mc / pref_bwd_mc / pref_bwd_mc_wide; the option
switches are those of ktup_set_option):

  case                 forward                                      backward
  generic  (36, 7)     pref_fwd_kernel<4,4> (d not a matrix-core    pref_bwd_kernel<4,4>: tile_front -> draw_uniform
                       width: pref_fwd_mc returns 1): draw_uniform
  row      (260, 7)    d > 256: pref_geom fails, pref_row_covers -> ktup_score_pref_row.hip row_uniform, both directions
  row_bwd  (100, 33)   n_pref > 32: pref_fwd_mc returns 1 ->        pg = ceil(33 / 2) = 17 > 16 -> pref_row on the padded tables
                       pref_fwd_kernel<7,4>
  mc       (64, 4)     pref_fwd_mc_kernel (HARD): per-wave noise    n <= bwd_wide_max -> pref_bwd_wide_kernel (four waves a tile),
           (100, 20)   fill, blocks shared by the 4 kq lanes;       its noise fill
           (100, 13)   P % 4 == 0 and != 0
  bwd_mc   same three  as mc                                        option bwd_wide_max = 0 -> pref_bwd_mc_kernel's noise fill
  wide256  (256, 20)   pref_fwd_mc at NCH = 64 (or the generic      d == 256 -> pref_bwd_wide_kernel, eight waves x 32 coordinates
           (256, 13)   <8,8> kernel where its LDS does not fit)
  valu     (100, 20)   option pref_mc = 0: pref_fwd_kernel<7,4> /   pref_bwd_kernel<7,4> / <8,8> (KSL-sliced at d = 256)
           (256, 13)   <8,8>
  steppers             RecStepper / JointStepper at d = 36: the launches above with KTUP_GUMBEL_PHILOX_DEV; at d = 100, and the
                       sharded step at d = 100 / 256: the STEP form of pref_bwd_wide_kernel (ktup_train_rec_step[_rows])

The score and training kernels form the noise with logf in BOTH modes (gumbel_from_uniform); the hardware-logarithm choice with a
logf redo inside a margin (gate_argmax in csrc/ktup_common.h, block-by-block for P % 4 == 0, index-by-index otherwise) is used by
csrc/ktup_eval.hip only, which tests/test_hip_eval.py ties to the host stream; test_eval_gate_across_the_32_bit_block_boundary adds
the offset those tests lack.  The close-call case below therefore checks that both modes of the score kernels settle a near tie
the same way, and that outside the margin the choice is the fp64 one."""
import copy

import pytest
import torch

from oracle import cpu_ref as O
from jTransUP.hip import lib as L
from tests.philox_host import uniforms

pytestmark = pytest.mark.gpu
DEV = 'cuda'
NU, NI, NE = 90, 70, 80
SEED = 0x9e3779b97f4a7c15 >> 1


class _opts(object):
    """with _opts(name=value, ...): library options for the duration of a block."""

    def __init__(self, **kv):
        self.kv = kv

    def __enter__(self):
        self.old = {k: L.set_option(k, v) for k, v in self.kv.items()}

    def __exit__(self, *exc):
        for k, v in self.old.items():
            L.set_option(k, v)


def ops():
    from jTransUP.hip import ops as _ops
    return _ops


def _world(seed, P, d):
    gen = torch.Generator().manual_seed(seed)
    mk = lambda r: O.make_table(r, d, gen)
    W = dict(U=mk(NU), I=mk(NI), E=torch.cat([mk(NE), torch.zeros(1, d)]), P=mk(P), Pn=mk(P), R=mk(P), Rn=mk(P))
    i2e = torch.randint(0, NE, (NI,), generator=gen)
    i2e[torch.rand(NI, generator=gen) < 0.1] = NE
    return W, i2e, gen


def _offsets(n, P):
    return [0, 4 * 555 + 3, 7, 2 ** 34 - (n * P) // 2 - 1]        # the last: the block index (offset + k) >> 2 crosses 2^32 inside the call


def _run(W, i2e, u, i, ktup, l1, mode, uni, seed, offset, weights):
    o = ops()
    names = ('U', 'I', 'E', 'P', 'Pn', 'R', 'Rn') if ktup else ('U', 'I', 'P', 'Pn')
    D = {k: W[k].to(DEV).clone().requires_grad_(True) for k in names}
    if ktup:
        s = o.score_ktup(D['U'], D['I'], D['E'], D['P'], D['Pn'], D['R'], D['Rn'], i2e.to(DEV, torch.int32), u, i, l1, mode, uni, seed, offset,
                         ent_pad=NE)
    else:
        s = o.score_tup(D['U'], D['I'], D['P'], D['Pn'], u, i, l1, mode, uni, seed, offset)
    (s * weights).sum().backward()
    return s.detach(), {k: D[k].grad for k in names}


def _compare(W, i2e, u, i, ktup, l1, seed, offset, weights):
    o = ops()
    n, P = u.numel(), W['P'].shape[0]
    uni = torch.from_numpy(uniforms(seed, offset, n * P).reshape(n, P)).to(DEV)
    sa, ga = _run(W, i2e, u, i, ktup, l1, o.GUMBEL_PHILOX, None, seed, offset, weights)
    sb, gb = _run(W, i2e, u, i, ktup, l1, o.GUMBEL_INPUT, uni, 0, 0, weights)
    what = 'ktup=%s n=%d offset=%d' % (ktup, n, offset)
    assert torch.equal(sa, sb), what
    for k in ga:
        torch.testing.assert_close(ga[k], gb[k], rtol=1e-4, atol=1e-5, msg=lambda m: '%s %s: %s' % (what, k, m))     # atomics order only
    # the forward VALUE of the gate is a one-hot, so pref_norm's (and norm's) gradient has exactly the rows some pair chose
    for k in ('Pn', 'Rn') if ktup else ('Pn',):
        rows_a, rows_b = (ga[k] != 0).any(dim=1), (gb[k] != 0).any(dim=1)
        assert torch.equal(rows_a, rows_b), '%s %s rows' % (what, k)
        assert int(rows_a.sum()) <= min(n, P)
    return sa


CASES = {
    'generic': (36, 7, {}),
    'row': (260, 7, {}),
    'row_bwd': (100, 33, {}),
    'mc_64_4': (64, 4, {}),
    'mc_100_20': (100, 20, {}),
    'mc_100_13': (100, 13, {}),
    'bwd_mc_64_4': (64, 4, {'bwd_wide_max': 0}),
    'bwd_mc_100_20': (100, 20, {'bwd_wide_max': 0}),
    'bwd_mc_100_13': (100, 13, {'bwd_wide_max': 0}),
    'wide256_20': (256, 20, {}),
    'wide256_13': (256, 13, {}),
    'valu_100_20': (100, 20, {'pref_mc': 0}),
    'valu_256_13': (256, 13, {'pref_mc': 0}),
}


@pytest.mark.parametrize('case', sorted(CASES))
def test_score_gate_draws_the_documented_stream(case):
    d, P, options = CASES[case]
    W, i2e, gen = _world(d + P, P, d)
    with _opts(**options):
        for n in (1, 17, 300):
            u = torch.randint(0, NU, (n,), generator=gen).to(DEV); i = torch.randint(0, NI, (n,), generator=gen).to(DEV)
            weights = torch.linspace(0.5, 1.5, n, device=DEV)
            seen = []
            last = _offsets(n, P)[-1]
            assert last >> 2 < 2 ** 32 <= (last + n * P - 1) >> 2
            for offset in _offsets(n, P):
                for ktup in (False, True):
                    seen.append(_compare(W, i2e, u, i, ktup, n == 17, SEED + n, offset, weights))
            assert n < 300 or not torch.equal(seen[0], seen[2])              # other offsets, other draws (TUP at offsets 0 and 2223)


@pytest.mark.parametrize('P', [20, 13])
def test_eval_gate_across_the_32_bit_block_boundary(P):
    """gate_argmax's two walks (csrc/ktup_common.h; reached from ktup_eval.hip) at an offset whose block index crosses 2^32."""
    d, nq = 64, 5
    W, _, gen = _world(P, P, d)
    D = {k: v.to(DEV) for k, v in W.items()}
    u = torch.randint(0, NU, (nq,), generator=gen).to(DEV)
    offset = 2 ** 34 - (nq * NI * P) // 2 - 1
    uni = torch.from_numpy(uniforms(SEED, offset, nq * NI * P).reshape(nq, NI, P)).to(DEV)
    o = ops()
    for l1 in (False, True):
        a = o.eval_tup(D['U'], D['I'], D['P'], D['Pn'], u, l1, o.GUMBEL_PHILOX, None, SEED, offset)
        b = o.eval_tup(D['U'], D['I'], D['P'], D['Pn'], u, l1, o.GUMBEL_INPUT, uni)
        assert torch.equal(a, b)


CLOSE_SEED, CLOSE_COUNT = 2, 7


def _close_calls(W, u, i, uni):
    """fp64: (lead of the winning preference over the runner-up, the winner's noisy logit) per pair, from the oracle's logits."""
    x = (W['U'][u] + W['I'][i]).double()
    logits = x @ W['P'].double().t() / 2                                       # oracle/cpu_ref.py tup_preferences
    un = torch.from_numpy(uni).double()
    v = logits - torch.log(-torch.log(un + 1e-20) + 1e-20)
    top = v.topk(2, dim=1).values
    return top[:, 0] - top[:, 1], top[:, 0]


def test_close_calls_are_settled_the_same_way():
    """d = 64, P = 20, 200,000 pairs: with CLOSE_SEED = 2 the host finds CLOSE_COUNT = 7 pairs whose winner leads the runner-up by no more
    than the redo margin 2e-5 + 2e-6 |best| of gate_argmax (fp64, oracle logits, host uniforms) -- a condition of the test, asserted.
    Philox and given-uniforms mode must agree on every one of them (scores bit for bit, gradients to the atomics bound), and outside
    the margin the scores are the oracle's for the same uniforms."""
    d, P, n = 64, 20, 200000
    W, _, gen = _world(1, P, d)
    u, i = torch.randint(0, NU, (n,), generator=gen), torch.randint(0, NI, (n,), generator=gen)
    offset = 4 * 31337 + 1
    uni = uniforms(CLOSE_SEED, offset, n * P).reshape(n, P)
    lead, best = _close_calls(W, u, i, uni)
    close = lead <= 2e-5 + 2e-6 * best.abs()
    count = int(close.sum())
    print('close calls: %d of %d pairs (smallest lead %.3g)' % (count, n, float(lead.min())))
    assert count >= 1 and count == CLOSE_COUNT
    weights = torch.linspace(0.5, 1.5, n, device=DEV) / n                    # a batch mean: gradients stay O(1) over 2e5 pairs
    got = _compare(W, None, u.to(DEV), i.to(DEV), False, False, CLOSE_SEED, offset, weights).cpu()
    want = O.score_tup(W['U'], W['I'], W['P'], W['Pn'], u, i, False, torch.from_numpy(uni))
    far = ~close
    torch.testing.assert_close(got[far], want[far], rtol=1e-4, atol=1e-5)


# ------------------------------------------------------------------------------------------------ steppers
def _tables_close(pairs, step):
    """tests/test_fast_train.py _assert_tables_close on (name, a, b) tensors."""
    from tests.test_fast_train import STRAY_CAP
    for k, a, b in pairs:
        err = (b - a).abs()
        bad = err > 2e-6 + 2e-5 * a.abs()
        assert float(bad.float().mean()) <= 2e-3 and float(err.max()) <= STRAY_CAP, \
            '%s after step %d: %d elements off, max %.3g' % (k, step, int(bad.sum()), float(err.max()))


@pytest.mark.parametrize('D', [36, 100])
@pytest.mark.parametrize('kind', ['transup', 'jtransup'])
def test_stepper_gate_draws_the_documented_stream(tmp_path, kind, D):
    """RecStepper (TUP) and JointStepper: three rec steps drawing from the device-resident stream against a twin fed, before step s,
    the host uniforms of positions s * 2 B P .. (s + 1) * 2 B P of the stepper's own seed: row k of [pos ; neg], preference p."""
    from jTransUP.models import transUP
    from jTransUP.utils.fast_train import JointStepper, RecStepper
    from tests.test_fast_train import _assert_tables_close, _trainer_for, build
    B, P = 64, 5
    if kind == 'jtransup':
        FLAGS, m1, tr1, (nu, ni, _, P) = build(tmp_path, 'Adagrad', True, D)
        _, m2, tr2, _ = build(tmp_path, 'Adagrad', True, D)
        Stepper = JointStepper
    else:
        nu, ni = 50, 40
        torch.manual_seed(4)
        m1, m2 = transUP.TransUPModel(False, D, nu, ni, P, True), transUP.TransUPModel(False, D, nu, ni, P, True)
        FLAGS, tr1 = _trainer_for(tmp_path, 'transup', m1)
        _, tr2 = _trainer_for(tmp_path, 'transup', m2)
        Stepper = RecStepper
    m2.load_state_dict(copy.deepcopy(m1.state_dict()))
    philox, twin = Stepper(m1, tr1, FLAGS, B, use_graphs=False), Stepper(m2, tr2, FLAGS, B, use_graphs=False)
    seed_used = int(philox.gstate[0])
    gen = torch.Generator().manual_seed(9)
    rnd = lambda hi: torch.randint(0, hi, (B,), generator=gen).to(DEV)
    for step in range(3):
        u, pi, ni_ = rnd(nu), rnd(ni), rnd(ni)
        assert philox.gstate.tolist() == [seed_used, step * 2 * B * P]
        twin.set_gumbel_uniforms(torch.from_numpy(uniforms(seed_used, step * 2 * B * P, 2 * B * P).reshape(2 * B, P)).to(DEV))
        la, lb = philox.rec_step(u, pi, ni_), twin.rec_step(u, pi, ni_)
        torch.testing.assert_close(la, lb, rtol=1e-5, atol=1e-6)
        _assert_tables_close(m1, m2, step)


@pytest.mark.parametrize('d', [100, 256])
def test_sharded_stepper_gate_draws_the_documented_stream(d):
    """ShardedKtupStepper on one rank (the fused step kernel exists for d in {64, 100, 128, 256} only: no d = 36 here), same scheme."""
    from jTransUP import parallel
    from jTransUP.sharded_ktup import ShardedKtupStepper
    nu, ni, ne, B, P = 300, 200, 250, 64, 20
    gen = torch.Generator().manual_seed(d)
    nrm = lambda r: torch.nn.functional.normalize(torch.randn(r, d, generator=gen), dim=1)
    full = {'U': nrm(nu), 'I': nrm(ni), 'E': nrm(ne)}
    small0 = [nrm(P) for _ in range(4)]
    i2e = torch.randint(0, ne, (ni,), generator=gen)
    i2e[::5] = -1
    dev = torch.device(DEV)

    def make():
        tabs = [parallel.ShardedTable(full[k].shape[0], d, rank=0, world=1, device=dev, init=lambda g, k=k: full[k][g].to(dev)) for k in 'UIE']
        small = [torch.nn.Parameter(t.clone().to(dev)) for t in small0]
        st = ShardedKtupStepper(*tabs, *small, i2e.to(torch.int32).to(dev), batch=B, kind='adagrad', lr=0.05, eps=1e-4, max_norm=0.5,
                                use_st_gumbel=True, gumbel_seed=5)
        return tabs, small, st
    (ta, sa, philox), (tb, sb, twin) = make(), make()
    seed_used = int(philox.gstate[0])
    for step in range(3):
        batch = [torch.randint(0, hi, (B,), generator=gen).to(dev) for hi in (nu, ni, ni)]
        assert philox.gstate.tolist() == [seed_used, step * 2 * B * P]
        twin.set_gumbel_uniforms(torch.from_numpy(uniforms(seed_used, step * 2 * B * P, 2 * B * P).reshape(2 * B, P)).to(dev))
        philox(*batch); twin(*batch)
        torch.cuda.synchronize()
        _tables_close([(k, a.weight.data, b.weight.data) for k, a, b in zip('UIE', ta, tb)] +
                      [('small%d' % k, a.data, b.data) for k, (a, b) in enumerate(zip(sa, sb))], step)
    assert philox.overflowed_steps() == 0 and twin.overflowed_steps() == 0
    torch.testing.assert_close(philox.loss_sum, twin.loss_sum, rtol=1e-5, atol=1e-6)
