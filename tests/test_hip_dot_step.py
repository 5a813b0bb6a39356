"""GPU parity of ktup_train_dot_step and ktup_reg_align_pairs (include/ktup_hip.h) through the C ABI: the kernels against fp64
torch on the CPU from the same fp32 inputs.  The tables are small so that rows collide: 7 users, 11 items, 6 rows of the second
item-side table of which the last is the pad row.

Tolerances are those of tests/test_hip_score.py: the loss rtol 1e-4; gradients (fp32 sums over the batch, atomics in any order)
rtol 1e-4 and atol max(3e-5, 2e-6 max|want|)."""
import itertools

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
DEV = 'cuda'
NU, NI, NX = 7, 11, 6
PAD = NX - 1


def lib():
    from jTransUP.hip import lib as L
    return L


def p(t):
    return None if t is None else t.data_ptr()


def close_grad(got, want, what):
    want = want.to(torch.float32)
    torch.testing.assert_close(got.cpu(), want, rtol=1e-4, atol=max(3e-5, 2e-6 * float(want.abs().max())), msg=lambda m: what + ': ' + m)


def make_case(B, d, bias, second, seed, pitch_extra=0):
    gen = torch.Generator().manual_seed(seed)
    ld = d + pitch_extra
    c = {'d': d, 'B': B, 'ld': ld}
    for name, rows in (('U', NU), ('I', NI), ('X', NX)):
        full = torch.randn(rows, ld, generator=gen) * 0.4
        c[name] = full
    c['X'][PAD] = 0.0                                               # what nn.Embedding(padding_idx) holds
    c['gbias'] = torch.randn(1, generator=gen) * 0.3 if bias else None
    c['bu'] = torch.randn(NU, generator=gen) * 0.3 if bias else None
    c['bi'] = torch.randn(NI, generator=gen) * 0.3 if bias else None
    if not second:
        c['X'] = None
    xmap = torch.randint(0, NX, (NI,), generator=gen)
    xmap[0] = PAD
    xmap[3] = PAD
    c['xmap'] = xmap if second else None
    c['u'] = torch.randint(0, NU, (B,), generator=gen)
    c['pi'] = torch.randint(0, NI, (B,), generator=gen)
    c['ni'] = torch.randint(0, NI, (B,), generator=gen)
    c['pi'][0] = 0                                                  # at least one pair on the pad row
    if B > 1:
        c['ni'][1] = 3
    return c


def reference(c, target, up):
    """fp64 on the CPU: (loss, {name: gradient}) of up * mean(-logsigmoid(target (s_pos - s_neg)))."""
    d = c['d']
    leaves = {}
    for k in ('U', 'I', 'X', 'bi'):
        if c[k] is not None:
            leaves[k] = c[k].double().clone().requires_grad_(True)
    U, I = leaves['U'][:, :d], leaves['I'][:, :d]

    def score(i):
        v = I[i]
        if c['X'] is not None:
            v = v + leaves['X'][:, :d][c['xmap'][i]]
        s = (U[c['u']] * v).sum(1)
        if c['gbias'] is not None:
            s = ((c['gbias'].double() + c['bu'].double()[c['u']]) + leaves['bi'][i]) + s
        return s

    loss = up * (-F.logsigmoid(target * (score(c['pi']) - score(c['ni'])))).mean()
    loss.backward()
    grads = {k: v.grad for k, v in leaves.items()}
    if 'X' in grads:
        grads['X'][PAD] = 0.0                                       # the pad row is gradient-free
    return float(loss.detach()), grads


def launch(c, target, up, bufs=None):
    L = lib()
    dev = {k: (None if c[k] is None else c[k].to(DEV)) for k in ('U', 'I', 'X', 'gbias', 'bu', 'bi', 'xmap')}
    u2 = torch.cat([c['u'], c['u']]).to(DEV)
    i2 = torch.cat([c['pi'], c['ni']]).to(DEV)
    if bufs is None:
        bufs = {'loss': torch.zeros(1, device=DEV), 'U': torch.zeros_like(dev['U']), 'I': torch.zeros_like(dev['I']),
                'X': None if dev['X'] is None else torch.zeros_like(dev['X']), 'bi': None if dev['bi'] is None else torch.zeros(NI, device=DEV)}
    ld = c['ld']
    for _ in range(bufs.setdefault('launches', 1)):
        L.call('ktup_train_dot_step', p(dev['U']), ld, p(dev['I']), ld, p(dev['X']), ld if dev['X'] is not None else 0, p(dev['xmap']),
               PAD if dev['X'] is not None else -1, p(dev['gbias']), p(dev['bu']), p(dev['bi']), c['d'], p(u2), p(i2), c['B'], float(target),
               float(up), p(bufs['loss']), p(bufs['U']), p(bufs['I']), p(bufs['X']), p(bufs['bi']), None)
    torch.cuda.synchronize()
    return bufs


def check(c, target, up, times=1):
    want_loss, want = reference(c, target, up)
    bufs = launch(c, target, up, None if times == 1 else {'launches': times, 'loss': torch.zeros(1, device=DEV),
                                                         'U': torch.zeros(NU, c['ld'], device=DEV), 'I': torch.zeros(NI, c['ld'], device=DEV),
                                                         'X': None if c['X'] is None else torch.zeros(NX, c['ld'], device=DEV),
                                                         'bi': None if c['bi'] is None else torch.zeros(NI, device=DEV)})
    got_loss = float(bufs['loss'].item())
    print('loss got %.9g want %.9g' % (got_loss, times * want_loss))
    torch.testing.assert_close(torch.tensor(got_loss, dtype=torch.float64), torch.tensor(times * want_loss, dtype=torch.float64),
                               rtol=1e-4, atol=0.0)
    for k in ('U', 'I', 'X', 'bi'):
        if bufs[k] is None:
            assert k not in want
            continue
        print(k, 'max |got - want| %.3g, max |want| %.3g' % (float((bufs[k].cpu().double() - times * want[k]).abs().max()),
                                                            float(want[k].abs().max())))
        close_grad(bufs[k], times * want[k], 'gradient of ' + k)
        if k in ('U', 'I', 'X') and c['ld'] > c['d']:
            assert float(bufs[k][:, c['d']:].abs().max()) == 0.0     # nothing lands between the rows
    if bufs['X'] is not None:
        assert float(bufs['X'][PAD].abs().max()) == 0.0             # exactly: never written
    return bufs


@pytest.mark.parametrize('d', [4, 36, 50, 100, 256])
@pytest.mark.parametrize('B', [1, 5, 64, 67])
def test_dot_step_shapes(B, d):
    """B below one workgroup's four examples, a full set of them, and a tail; d = 50 takes the element-wise path."""
    check(make_case(B, d, bias=True, second=True, seed=100 * B + d), 1.0, 1.0)


@pytest.mark.parametrize('d', [36, 100])
@pytest.mark.parametrize('bias,second,target', list(itertools.product([False, True], [False, True], [1.0, -1.0])))
def test_dot_step_options(d, bias, second, target):
    check(make_case(67, d, bias=bias, second=second, seed=7 * d + 2 * bias + second), target, 0.5)


def test_dot_step_with_padded_rows():
    """Pitches d + 4 (rows stay 16-byte aligned: the float4 path with a gap between the rows), and d + 1 (element-wise)."""
    check(make_case(67, 36, bias=True, second=True, seed=5, pitch_extra=4), 1.0, 1.0)
    check(make_case(67, 36, bias=True, second=True, seed=6, pitch_extra=1), -1.0, 1.0)


def test_dot_step_adds_to_its_outputs():
    """A second launch into the same buffers doubles them: the kernel adds, it does not store."""
    check(make_case(64, 100, bias=True, second=True, seed=11), 1.0, 1.0, times=2)


@pytest.mark.parametrize('l1', [1, 0])
@pytest.mark.parametrize('d', [5, 36])
@pytest.mark.parametrize('n', [0, 1, 9])
def test_align_pairs(n, d, l1):
    L = lib()
    cap, NA, NB, scale = 16, 6, 8, 0.7
    gen = torch.Generator().manual_seed(50 * n + d + l1)
    A, B = torch.randn(NA, d, generator=gen), torch.randn(NB, d, generator=gen)
    a_ids, b_ids = torch.randint(0, NA, (cap,), generator=gen), torch.randint(0, NB, (cap,), generator=gen)
    a_ids[0], b_ids[0] = 2, 5
    B[5] = A[2]                                                     # a pair of identical rows: sign(0) = 0 under L1
    if n > 2:
        a_ids[3], b_ids[4] = a_ids[1], b_ids[2]                     # duplicate ids on either side
    Ad, Bd = A.double().requires_grad_(True), B.double().requires_grad_(True)
    gA0, gB0 = torch.randn(NA, d, generator=gen), torch.randn(NB, d, generator=gen)
    want_loss, want_gA, want_gB = 0.25, gA0.double().clone(), gB0.double().clone()
    if n:
        z = Ad[a_ids[:n]] - Bd[b_ids[:n]]
        term = scale * (z.abs().sum(1) if l1 else (z ** 2).sum(1)).mean()
        term.backward()
        want_loss, want_gA, want_gB = want_loss + float(term), want_gA + Ad.grad, want_gB + Bd.grad
    loss = torch.full((1,), 0.25, device=DEV)
    gA, gB = gA0.to(DEV), gB0.to(DEV)
    n_dev = torch.tensor([n], dtype=torch.int64, device=DEV)
    dA, dB, da, db = A.to(DEV), B.to(DEV), a_ids.to(DEV), b_ids.to(DEV)
    for n_host in (-1, n):                                          # the captured form (length on the device only) and the eager one
        loss.fill_(0.25); gA.copy_(gA0); gB.copy_(gB0)
        L.call('ktup_reg_align_pairs', p(dA), d, p(dB), d, d, p(da), p(db), p(n_dev), n_host, cap, l1, scale, p(loss), p(gA), p(gB), None)
        torch.cuda.synchronize()
        if n == 0:                                                  # untouched, exactly
            assert float(loss.item()) == 0.25 and torch.equal(gA.cpu(), gA0) and torch.equal(gB.cpu(), gB0)
            continue
        print('loss got %.9g want %.9g' % (float(loss.item()), want_loss))
        torch.testing.assert_close(torch.tensor(float(loss.item()), dtype=torch.float64), torch.tensor(want_loss, dtype=torch.float64),
                                   rtol=1e-4, atol=0.0)
        close_grad(gA, want_gA, 'gA')
        close_grad(gB, want_gB, 'gB')
        if l1:
            assert n > 1 or torch.equal(gA.cpu(), gA0)              # n = 1 is the identical pair alone: no gradient at all


def test_align_pairs_clamps_the_device_length_to_the_capacity():
    """*n_dev beyond cap (a host that could not know): the kernel reads cap pairs, never past the buffers."""
    L = lib()
    cap, d = 4, 5
    gen = torch.Generator().manual_seed(1)
    A, B = torch.randn(3, d, generator=gen), torch.randn(3, d, generator=gen)
    ids = torch.tensor([0, 1, 2, 1])
    want = 2.0 * (A.double()[ids] - B.double()[ids]).abs().sum(1).mean()
    loss, gA, gB = torch.zeros(1, device=DEV), torch.zeros(3, d, device=DEV), torch.zeros(3, d, device=DEV)
    n_dev = torch.tensor([1000], dtype=torch.int64, device=DEV)
    dA, dB, di = A.to(DEV), B.to(DEV), ids.to(DEV)
    L.call('ktup_reg_align_pairs', p(dA), d, p(dB), d, d, p(di), p(di), p(n_dev), -1, cap, 1, 2.0, p(loss), p(gA), p(gB), None)
    torch.cuda.synchronize()
    torch.testing.assert_close(float(loss.item()), float(want), rtol=1e-4, atol=0.0)
