"""ktup_feed_remap_ids and ktup_feed_align_lists (csrc/ktup_feed_joint.hip) through the C ABI.  Integer results compare exactly.
The oracle of the alignment lists is what the drivers run on the host: getMappedEntities / getMappedItems on the vocabulary
construction of tests/test_fast_train_dot.py (`world_maps`, copied here with the sizes as arguments: the small 40 / 70 world and one
large enough for 16,384 distinct aligned ids)."""
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda', 0)
FILL = -7                       # what the list buffers hold before a launch: entries past n must keep it


def lib():
    from jTransUP.hip import lib as L
    return L


def p(t):
    return None if t is None else t.data_ptr()


def stream():
    return torch.cuda.current_stream().cuda_stream


def dev(x):
    return torch.tensor(x, dtype=torch.int64, device=DEV)


def world_maps(NI, NE):
    """Items 0, 5, 10, ... have no entity; the others map to distinct entities (NE is no multiple of 3, NI <= NE); entities no item
    maps to have a key of their own."""
    i_map = {i: 'k%d' % i for i in range(NI)}
    ikg = {'k%d' % i: ((i * 3) % NE if i % 5 else -1, i) for i in range(NI)}
    e_map = {e: 'e%d' % e for e in range(NE)}
    for key, (e, i) in list(ikg.items()):
        if e != -1:
            e_map[e] = key
    for e in range(NE):
        if e_map[e] == 'e%d' % e:
            ikg['e%d' % e] = (e, -1)
    return i_map, e_map, ikg


class World(object):
    def __init__(self, NI, NE):
        self.NI, self.NE = NI, NE
        self.i_map, self.e_map, self.ikg = world_maps(NI, NE)
        # raw id -> aligned id of the other space, or -1: [0] keyed by items, [1] keyed by entities
        self.partner = (dev([self.ikg[self.i_map[i]][0] for i in range(NI)]), dev([self.ikg[self.e_map[e]][1] for e in range(NE)]))

    def oracle(self, ids, ent):
        from jTransUP.models.knowledgable_recommendation import getMappedEntities, getMappedItems
        e_ids, i_ids = getMappedItems(ids, self.e_map, self.ikg) if ent else getMappedEntities(ids, self.i_map, self.ikg)
        return sorted(zip(e_ids, i_ids))

    def n_ids(self, ent):
        return self.NE if ent else self.NI


@pytest.fixture(scope='module')
def small():
    return World(40, 70)


@pytest.fixture(scope='module')
def large():
    return World(24000, 30001)           # 19,200 aligned items: room for 16,384 distinct aligned ids in either direction


def max_ids():
    so, n = lib().load(), 1
    while so.ktup_feed_align_lists_supported(2 * n):
        n *= 2
    return n


def align(world, a, b, ent, cap=None):
    """One launch on fresh buffers -> (n, sorted pairs, the two list buffers)."""
    L = lib()
    na, nb = len(a), 0 if b is None else len(b)
    cap = na + nb if cap is None else cap
    ta, tb = dev(a), None if b is None else dev(b)
    n_out = dev([FILL])
    e_ids, i_ids = torch.full((cap,), FILL, dtype=torch.int64, device=DEV), torch.full((cap,), FILL, dtype=torch.int64, device=DEV)
    tab = world.partner[ent]
    L.call('ktup_feed_align_lists', p(ta), na, p(tb), nb, p(tab), tab.numel(), ent, cap, p(n_out), p(e_ids), p(i_ids), None, stream())
    torch.cuda.synchronize()
    n = int(n_out.item())
    assert 0 <= n <= na + nb
    e, i = e_ids.tolist(), i_ids.tolist()
    assert all(x == FILL for x in e[n:]) and all(x == FILL for x in i[n:]), 'wrote past the list'
    return n, sorted(zip(e[:n], i[:n])), e, i


def check(world, a, b, ent):
    n, pairs, _, _ = align(world, a, b, ent)
    want = world.oracle(list(a) + list(b or []), ent)
    assert n == len(want)
    assert pairs == want
    return n


def totals():
    return [1, 2, 63, 64, 65, 1023, 1024, 1025, 1600, max_ids()]


# ---------------------------------------------------------------------------------------------------- remap
@pytest.mark.parametrize('with_b', [False, True])
@pytest.mark.parametrize('na', [1, 64, 65, 1025])
def test_remap_equals_indexing_the_table(na, with_b):
    L = lib()
    gen = torch.Generator().manual_seed(100 + na + int(with_b))
    n_map = 300
    table = torch.randperm(1000, generator=gen)[:n_map].to(DEV)
    nb = na + 3 if with_b else 0
    a = torch.randint(0, n_map, (na,), generator=gen).to(DEV)
    b = torch.randint(0, n_map, (nb,), generator=gen).to(DEV) if with_b else None
    want_a, want_b = table[a], None if b is None else table[b]
    fail = torch.zeros(1, dtype=torch.int32, device=DEV)
    L.call('ktup_feed_remap_ids', p(table), n_map, p(a), na, p(b), nb, p(fail), stream())
    torch.cuda.synchronize()
    assert torch.equal(a, want_a)
    if with_b:
        assert torch.equal(b, want_b)
    assert int(fail.item()) == 0


@pytest.mark.parametrize('case', ['out-of-range id', 'negative entry'])
def test_remap_stands_in_row_zero_and_counts(case):
    L = lib()
    gen = torch.Generator().manual_seed(7)
    n_map = 50
    table = (torch.randperm(n_map, generator=gen) + 11)
    a = torch.randint(0, n_map, (65,), generator=gen)
    b = torch.randint(0, n_map, (64,), generator=gen)
    if case == 'out-of-range id':
        a[3], a[64], b[0], b[63] = n_map, -1, n_map + 1000, -(1 << 40)
        bad_a, bad_b = [3, 64], [0, 63]
    else:
        table[5], table[17] = -1, -9
        a[10], a[11], b[20] = 5, 17, 5
        bad_a = [k for k in range(65) if int(a[k]) in (5, 17)]
        bad_b = [k for k in range(64) if int(b[k]) in (5, 17)]
    want_a = [0 if k in bad_a else int(table[a[k]]) for k in range(65)]
    want_b = [0 if k in bad_b else int(table[b[k]]) for k in range(64)]
    table, a, b = table.to(DEV), a.to(DEV), b.to(DEV)
    fail = torch.zeros(1, dtype=torch.int32, device=DEV)
    L.call('ktup_feed_remap_ids', p(table), n_map, p(a), 65, p(b), 64, p(fail), stream())
    torch.cuda.synchronize()
    assert a.tolist() == want_a and b.tolist() == want_b
    assert int(fail.item()) == len(bad_a) + len(bad_b)
    L.call('ktup_feed_remap_ids', p(table), n_map, p(a[:1]), 1, None, 0, None, stream())      # the counter is optional
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------- alignment lists
@pytest.mark.parametrize('ent', [0, 1])
@pytest.mark.parametrize('which', range(10))
def test_align_lists_equal_the_host_lists(small, large, which, ent):
    """Random ids with repeats, split over a and b, from a range that reaches past n_partner (those are skipped)."""
    total = totals()[which]
    world = small if total <= 65 else large
    gen = torch.Generator().manual_seed(1000 * ent + total)
    if total == 2:
        ids = [7, 7]                                                     # 2 (equal)
    else:
        hi = world.n_ids(ent) + 9 if total <= 65 else min(world.n_ids(ent) + 9, max(8, total))
        ids = torch.randint(0, hi, (total,), generator=gen).tolist()
    na = total - total // 3
    n = check(world, ids[:na], ids[na:] or None, ent)
    print('total %d, ent %d: %d pairs' % (total, ent, n))
    assert total == 1 or n < total


@pytest.mark.parametrize('ent', [0, 1])
@pytest.mark.parametrize('total', [64, 1025])
def test_all_ids_equal(small, total, ent):
    aligned, unaligned = (6, 5) if not ent else (3, 1)                   # item 6 <-> entity 18, item 1 <-> entity 3; item 5, entity 1: none
    assert check(small, [aligned] * (total - 20), [aligned] * 20, ent) == 1
    assert check(small, [unaligned] * total, None, ent) == 0


@pytest.mark.parametrize('ent', [0, 1])
@pytest.mark.parametrize('which', [3, 7, 9])
def test_all_distinct_and_all_aligned_fills_the_list_exactly(large, which, ent):
    total = totals()[which]                                              # 64, 1025, the maximum
    items = [i for i in range(large.NI) if i % 5][:total]
    ids = [(i * 3) % large.NE for i in items] if ent else items
    gen = torch.Generator().manual_seed(total)
    ids = [ids[k] for k in torch.randperm(total, generator=gen).tolist()]
    na = total // 2 + 1
    assert check(large, ids[:na], ids[na:], ent) == total               # n == na + nb == cap


@pytest.mark.parametrize('ent', [0, 1])
def test_no_id_aligned_leaves_the_buffers_untouched(small, ent):
    lone = [i for i in range(small.n_ids(ent)) if int(small.partner[ent][i]) < 0]
    ids = (lone * 40)[:130] + [small.n_ids(ent), small.n_ids(ent) + 5, 1 << 40, -1, -(1 << 35)]
    n, pairs, e, i = align(small, ids[:70], ids[70:], ent, cap=200)
    assert n == 0 and pairs == [] and e == [FILL] * 200 and i == [FILL] * 200


@pytest.mark.parametrize('ent', [0, 1])
@pytest.mark.parametrize('total', [65, 1600])
def test_b_may_be_null(small, large, total, ent):
    world = small if total == 65 else large
    gen = torch.Generator().manual_seed(31 * total + ent)
    ids = torch.randint(0, min(world.n_ids(ent), 3 * total), (total,), generator=gen).tolist()
    check(world, ids, None, ent)


@pytest.mark.parametrize('total', [1600, None])
def test_replays_rebuild_the_table(large, total):
    """Captured once, replayed four times with the id buffer rewritten in between: every replay gives the host's lists -- nothing of
    one launch's dedupe table reaches the next."""
    L = lib()
    total = max_ids() if total is None else total
    ent, na = 1, total // 2
    tab = large.partner[ent]
    ids = torch.zeros(total, dtype=torch.int64, device=DEV)
    n_out = dev([FILL])
    e_ids, i_ids = (torch.full((total,), FILL, dtype=torch.int64, device=DEV) for _ in range(2))
    graph = torch.cuda.CUDAGraph()
    with L.capture(graph):
        L.call('ktup_feed_align_lists', p(ids), na, p(ids[na:]), total - na, p(tab), tab.numel(), ent, total, p(n_out), p(e_ids), p(i_ids),
               None, stream())
    torch.cuda.synchronize()
    gen = torch.Generator().manual_seed(77)
    for replay in range(4):
        hi = (8, large.NE, total // 4, large.NE + 9)[replay]             # many repeats, few, some, ids past the table
        fresh = torch.randint(0, hi, (total,), generator=gen)
        ids.copy_(fresh)
        torch.cuda.synchronize()
        graph.replay()
        torch.cuda.synchronize()
        n = int(n_out.item())
        want = large.oracle(fresh.tolist(), ent)
        assert n == len(want), 'replay %d' % replay
        assert sorted(zip(e_ids[:n].tolist(), i_ids[:n].tolist())) == want, 'replay %d' % replay


@pytest.mark.parametrize('ent', [0, 1])
def test_lists_feed_the_alignment_term(small, ent):
    """ktup_feed_align_lists -> ktup_reg_align_pairs (list length read on the device) against pNormLoss on the host-built lists through
    autograd: squared L2, d = 20; the bar of tests/test_fast_train_dot.py::test_dot_steppers_match_the_autograd_route."""
    from jTransUP.utils.loss import pNormLoss
    L = lib()
    d, cap, scale = 20, 64, 0.7
    gen = torch.Generator().manual_seed(5 + ent)
    E = torch.randn(small.NE, d, generator=gen).to(DEV)
    I = torch.randn(small.NI, d, generator=gen).to(DEV)
    ids = torch.randint(0, small.n_ids(ent), (48,), generator=gen)
    a, b = ids[:32].to(DEV), ids[32:].to(DEV)
    buf = torch.zeros(1 + 2 * cap, dtype=torch.int64, device=DEV)       # [n | entity ids (cap) | item ids (cap)]
    loss = torch.zeros(1, device=DEV)
    gE, gI = torch.zeros_like(E), torch.zeros_like(I)
    tab = small.partner[ent]
    L.call('ktup_feed_align_lists', p(a), 32, p(b), 16, p(tab), tab.numel(), ent, cap, p(buf), p(buf[1:]), p(buf[1 + cap:]), None, stream())
    L.call('ktup_reg_align_pairs', p(E), E.stride(0), p(I), I.stride(0), d, p(buf[1:]), p(buf[1 + cap:]), p(buf), -1, cap, 0, scale,
           p(loss), p(gE), p(gI), stream())
    torch.cuda.synchronize()
    want = small.oracle(ids.tolist(), ent)
    assert int(buf[0]) == len(want) > 4
    Eh, Ih = E.cpu().requires_grad_(True), I.cpu().requires_grad_(True)
    ref = scale * pNormLoss(Eh[torch.tensor([e for e, _ in want])], Ih[torch.tensor([i for _, i in want])], L1_flag=False)
    ref.backward()
    print('loss %.9g (autograd %.9g)' % (float(loss), float(ref)))
    torch.testing.assert_close(loss.cpu().reshape(()), ref.detach(), rtol=1e-5, atol=1e-6)
    torch.testing.assert_close(gE.cpu(), Eh.grad, rtol=1e-5, atol=1e-6)
    torch.testing.assert_close(gI.cpu(), Ih.grad, rtol=1e-5, atol=1e-6)
