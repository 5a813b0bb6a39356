"""GPU parity of the sharded step's launches (csrc/ktup_shard_step.hip and the segment walk of csrc/ktup_segreduce.hip) through the C
ABI (jTransUP.hip.lib.call on raw pointers) against tests/_shard_ref.py: fp64 from the same fp32 inputs, at tolerances derived in
that module and pinned on the CPU by tests/test_shard_ref_host.py.  The route is checked by invariants (slots are handed out in
atomic arrival order); the reduction walks run on geometries made exact by routing ids 0 .. 63 with world = 64 and cap = 1
(tests/_shard_cases.py): segment layouts against chunk and workgroup-stretch edges at one embedding size per template rung and
edge.  Every device buffer sits between guard bytes that must come back bit-identical.  Each case prints its largest
error / tolerance; test_zz_report prints the largest per entry point.

Kept preconditions (never probed): phase 2 / 5 only on scratch phase 1 / 4 filled in the same test; ids < 2^56; a reduce call only
gets the sort_ws of a route call with the same n_entries and W; the current stream, no graphs.

Rows that owe steps (last < t - 1; Adam's zero-gradient replay and, under weight decay, rules 0 / 1 / 2 on wd * p) are part of both apply
tests (the `stale` option sets) and of test_adam_catchup; the small replicated tables always carry last = t - 1.

Not covered: wire buffers near 2^31 rows, n_entries >= 73,728 (where the chunk grows), the exchange between ranks (the stepper
tests), Adam replays of young states (the existing flush test), owed steps on the small tables, rows never written (last = 0) under
weight decay (they owe every step since the first; the stepper tests run that at small step counts)."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from tests import _shard_cases as C
from tests import _shard_ref as R

pytestmark = pytest.mark.gpu
DEV = 'cuda'
GUARD = 64                                                            # bytes on each side of every device buffer
WORST = {}                                                            # entry point -> largest error / tolerance of the module


class AdamRule(ctypes.Structure):                                     # ktup_adam_t (include/ktup_hip.h)
    _fields_ = [('beta1', ctypes.c_float), ('beta2', ctypes.c_float), ('replay', ctypes.c_int32), ('rule', ctypes.c_int32),
                ('step', ctypes.c_void_p), ('weight_decay', ctypes.c_float), ('reserved', ctypes.c_float)]


# ------------------------------------------------------------------------------------------------ plumbing
def lib():
    from jTransUP.hip import lib as L
    return L


def call(name, *args):
    lib().call(name, *args)


def refused(name, *args):
    """(status, message) of a call that must be refused before any launch."""
    raw = lib().load()
    rc = getattr(raw, name)(*args)
    return rc, raw.ktup_last_error().decode('utf-8', 'replace')


def stream():
    return torch.cuda.current_stream().cuda_stream


def arr(ctype, vals):
    vals = list(vals)
    return (ctype * max(len(vals), 1))(*vals)


def i64(vals):
    return arr(ctypes.c_int64, [int(v) for v in vals])


def ptrs(handles):
    return arr(ctypes.c_void_p, [None if h is None else h.ptr for h in handles])


def note(name, ratio):
    cur = WORST.get(name, 0.0)
    WORST[name] = ratio if not ratio <= cur else cur                    # (keeps a NaN)


LIVE = []                                                             # every device buffer the running test made
TOUCHED = []                                                          # the shared routes (routed) it used


class Buf:
    """A device buffer between GUARD bytes of 0xA5 on either side."""

    def __init__(self, host):
        host = np.ascontiguousarray(host)
        self.dtype, self.shape, self.nbytes = host.dtype, host.shape, host.nbytes
        raw = np.full(2 * GUARD + host.nbytes, 0xA5, np.uint8)
        raw[GUARD:GUARD + host.nbytes] = host.reshape(-1).view(np.uint8)
        self.t = torch.from_numpy(raw).to(DEV)
        self.ptr = self.t.data_ptr() + GUARD
        assert self.ptr % 64 == 0
        LIVE.append(self)

    def guards(self):
        torch.cuda.synchronize()
        assert bool((self.t[:GUARD] == 0xA5).all()) and bool((self.t[GUARD + self.nbytes:] == 0xA5).all()), 'guard bytes overwritten'

    def get(self):
        """The buffer's contents; its guards must be intact."""
        self.guards()
        return self.t[GUARD:GUARD + self.nbytes].cpu().numpy().view(self.dtype).reshape(self.shape)


@pytest.fixture(autouse=True)
def every_guard_is_intact():
    """After each test: the guard bytes of every buffer it made, read or not, and of the routes shared between tests."""
    first = len(LIVE)
    del TOUCHED[:]
    yield
    for h in LIVE[first:] + [h for r in TOUCHED for h in r.values() if h is not None]:
        h.guards()
    del LIVE[first:]


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


# ------------------------------------------------------------------------------------------------ route
def route(rc):
    """ktup_shard_route on a case; every output in a prefilled, guarded buffer.  Returns the buffers."""
    L = lib().load()
    ids = rc['ids']
    n = len(ids)
    T, world = len(rc['cap']), rc['world']
    _, _, _, W = R.wire(world, rc['cap'])
    lay = R.sort_layout(n, W)
    assert L.ktup_shard_route_sort_bytes(n, W) == 4 * lay['len']
    b = {'ids': Buf(ids), 'inverse': Buf(np.full(n, -9, np.int64)), 'send_ids': Buf(np.full(W, -5, np.int64)),
         'pair_map': Buf(np.full(W + 1, -7, np.int32)) if rc['pair'] else None, 'sort_ws': Buf(np.full(lay['len'], -3, np.int32)),
         'counters': Buf(np.full(world * T + 1, 77, np.int32)), 'zero': Buf(np.full(3, np.nan)),
         'ws': Buf(np.full(L.ktup_shard_route_workspace_bytes(n), 0x5A, np.uint8))}
    pa, pb = rc['pair'] or (0, 0)
    call('ktup_shard_route', b['ids'].ptr, n, rc['block'], T, i64(rc['ent_off']), world, i64(rc['cap']), pa, pb, b['inverse'].ptr,
         b['send_ids'].ptr, b['pair_map'].ptr if rc['pair'] else None, b['sort_ws'].ptr, b['counters'].ptr, b['zero'].ptr, 3,
         b['ws'].ptr, stream())
    return b


def check_routed(rc, b, ids=None):
    out = {k: (v.get() if v is not None else None) for k, v in b.items()}
    assert np.array_equal(out['ids'], rc['ids'] if ids is None else ids), 'the entry list changed'
    assert not out['zero'].view(np.uint64).any(), 'zero_doubles must be cleared (+0.0)'
    pa, pb = rc['pair'] or (1, 2)
    R.check_route(out['ids'], rc['block'], rc['ent_off'], rc['world'], rc['cap'], out['inverse'], out['send_ids'], out['pair_map'],
                  out['counters'], out['sort_ws'], pa, pb)
    return out


@pytest.mark.parametrize('name', C.ROUTES + C.OVERFLOW, ids=str)
def test_route(name):
    """T in 1 .. 4 x world in {1, 2, 3, 64}; the owner-side form (world = 1, block = capsum, one row asked by many peers); 10 distinct
    ids over 5,000 entries; all distinct; all padding; one entry; one numeric id in two tables (two rows); ids near 2^40; distinct ==
    cap; pair_map; overflow by 1 and by many per owner (counted, every inverse still inside the buffer, nothing outside written)."""
    rc = C.route_case(name)
    out = check_routed(rc, route(rc))
    if name[0] == 'overflow':
        assert int(out['counters'][-1]) == 2 * name[1]
    if name[0] == 'same_id_two_tables':
        rows = {int(w) for w in out['inverse'][rc['ids'] >= 0]}
        assert len(rows) == 4                                              # ids 5 and 9 in each of the two tables


@pytest.mark.parametrize('name', C.SCAN, ids=str)
def test_route_scan_paths(name):
    """W = 1, 3, 1023, 1024, 1025, 4098 (the tile tail, W % 4 != 0), 262,145 (more than 256 tiles: two tile totals per thread in
    the scatter launch) and 1,048,580 (past MAX_TILES: the one-workgroup wide scan); at most 4,096 entries each."""
    rc = C.route_case(name)
    assert len(rc['ids']) <= 4096 + 37
    check_routed(rc, route(rc))


def _ktup_route(kb, cursor, phases, bufs=None):
    """ktup_shard_route_ktup over the id columns; phases run one after the other on the same buffers and stream."""
    L = lib().load()
    B, T = kb['B'], 3 if kb['item2ent'] is not None else 2
    n = (5 if T == 3 else 3) * B
    _, _, _, W = R.wire(kb['world'], kb['cap'])
    lay = R.sort_layout(n, W)
    b = bufs or {'u': Buf(kb['u']), 'pos': Buf(kb['pos']), 'neg': Buf(kb['neg']),
                 'item2ent': Buf(kb['item2ent']) if T == 3 else None, 'cursor': Buf(np.asarray([7, cursor, 7], np.int64)),
                 'ids': Buf(np.full(n, -11, np.int64)), 'inverse': Buf(np.full(n, -9, np.int64)), 'send_ids': Buf(np.full(W, -5, np.int64)),
                 'pair_map': Buf(np.full(W + 1, -7, np.int32)) if T == 3 else None, 'sort_ws': Buf(np.full(lay['len'], -3, np.int32)),
                 'counters': Buf(np.full(kb['world'] * T + 1, 77, np.int32)), 'zero': Buf(np.full(3, np.nan)),
                 'ws': Buf(np.full(L.ktup_shard_route_workspace_bytes(n), 0x5A, np.uint8))}
    for phase in phases:
        call('ktup_shard_route_ktup', b['u'].ptr, b['pos'].ptr, b['neg'].ptr, B, kb['n_batches'], b['cursor'].ptr + 8,
             b['item2ent'].ptr if T == 3 else None, kb['ent_pad'], b['ids'].ptr, kb['world'], i64(kb['cap']), b['inverse'].ptr,
             b['send_ids'].ptr, b['pair_map'].ptr if T == 3 else None, b['sort_ws'].ptr, b['counters'].ptr, b['zero'].ptr, 3, b['ws'].ptr,
             phase, stream())
    return b


def _ktup_rc(kb, batch):
    ids = R.ktup_entries_model(kb['u'][batch], kb['pos'][batch], kb['neg'][batch], kb['item2ent'], kb['ent_pad'])
    B, T = kb['B'], 3 if kb['item2ent'] is not None else 2
    return {'ids': ids, 'block': len(ids), 'ent_off': np.asarray([0, B, 3 * B, 5 * B][:T + 1], np.int64), 'world': kb['world'],
            'cap': kb['cap'], 'pair': (1, 2) if T == 3 else None}


ROUTE_KEYS = ('ids', 'inverse', 'send_ids', 'pair_map', 'sort_ws', 'counters', 'zero', 'ws')


@pytest.mark.parametrize('with_ent', [True, False], ids=['item2ent', 'no_item2ent'])
@pytest.mark.parametrize('phases', [(0,), (1, 2), (4, 5), (3,)], ids=str)
def test_route_ktup(phases, with_ent):
    """The entry list built by the first launch ([u | pos ; neg | item2ent[pos ; neg]], an entity of -1 or ent_pad becoming padding; 3B
    entries and two tables without item2ent) equals ktup_shard_ktup_entries and the numpy model; the cursor walks three batches and
    wraps, moved once by phase 0, by 1 + 2 and by 4 + 5, left alone by phase 3; every phase split gives the same checked route."""
    kb = C.ktup_batches(with_ent=with_ent)
    b, cursor = None, 1
    for _ in range(4):                                                    # batches 1, 2, 0, 1
        b = _ktup_route(kb, cursor, phases, b)
        batch = cursor % kb['n_batches']
        rc = _ktup_rc(kb, batch)
        check_routed(rc, {k: b[k] for k in ROUTE_KEYS}, ids=rc['ids'])
        moved = 0 if phases == (3,) else 1
        assert b['cursor'].get().tolist() == [7, cursor + moved, 7]
        ent = Buf(np.full(len(rc['ids']), -11, np.int64))
        off = 8 * batch * kb['B']
        call('ktup_shard_ktup_entries', b['u'].ptr + off, b['pos'].ptr + off, b['neg'].ptr + off, kb['B'],
             b['item2ent'].ptr if with_ent else None, kb['ent_pad'], ent.ptr, stream())
        assert np.array_equal(ent.get(), rc['ids'])
        if moved == 0:                                                    # phase 3: the caller moves the cursor (ktup_shard_reduce_norm does)
            b['cursor'] = Buf(np.asarray([7, cursor + 1, 7], np.int64))
        cursor += 1
        for k in ('u', 'pos', 'neg'):
            assert np.array_equal(b[k].get(), kb[k])


@pytest.mark.parametrize('phases', [(0,), (1, 2), (4, 5), (3,)], ids=str)
def test_route_kg(phases):
    """entries = [ph ; pt ; nh ; nt] with the twins nh == ph / nt == pt as -1, rels = [pr ; nr], one table; the cursor as above."""
    L = lib().load()
    kb = C.kg_batches()
    B, n = kb['B'], 4 * kb['B']
    _, _, _, W = R.wire(kb['world'], kb['cap'])
    lay = R.sort_layout(n, W)
    b = {k: Buf(kb[k]) for k in ('ph', 'pt', 'pr', 'nh', 'nt', 'nr')}
    b.update({'ids': Buf(np.full(n, -11, np.int64)), 'rels': Buf(np.full(2 * B, -11, np.int64)), 'inverse': Buf(np.full(n, -9, np.int64)),
              'send_ids': Buf(np.full(W, -5, np.int64)), 'pair_map': None, 'sort_ws': Buf(np.full(lay['len'], -3, np.int32)),
              'counters': Buf(np.full(kb['world'] + 1, 77, np.int32)), 'zero': Buf(np.full(3, np.nan)),
              'ws': Buf(np.full(L.ktup_shard_route_workspace_bytes(n), 0x5A, np.uint8))})
    cursor = 1
    for _ in range(3):                                                    # batches 1, 0, 1
        b['cursor'] = Buf(np.asarray([7, cursor, 7], np.int64))
        for phase in phases:
            call('ktup_shard_route_kg', b['ph'].ptr, b['pt'].ptr, b['pr'].ptr, b['nh'].ptr, b['nt'].ptr, b['nr'].ptr, B, kb['n_batches'],
                 b['cursor'].ptr + 8, b['ids'].ptr, b['rels'].ptr, kb['world'], i64(kb['cap']), b['inverse'].ptr, b['send_ids'].ptr,
                 b['sort_ws'].ptr, b['counters'].ptr, b['zero'].ptr, 3, b['ws'].ptr, phase, stream())
        batch = cursor % kb['n_batches']
        ids, rels = R.kg_entries_model(*(kb[k][batch] for k in ('ph', 'pt', 'pr', 'nh', 'nt', 'nr')))
        assert (ids[2 * B:] == -1).sum() >= B                             # every corrupted triple keeps its head or its tail
        rc = {'ids': ids, 'block': n, 'ent_off': np.asarray([0, n], np.int64), 'world': kb['world'], 'cap': kb['cap'], 'pair': None}
        check_routed(rc, {k: b[k] for k in ROUTE_KEYS}, ids=ids)
        assert np.array_equal(b['rels'].get(), rels)
        assert b['cursor'].get().tolist() == [7, cursor + (0 if phases == (3,) else 1), 7]
        cursor += 1


# ------------------------------------------------------------------------------------------------ the reduction walks
CASES, case_id = C.CASES, C.case_id


def routed(case):
    """The case routed once on the GPU (shared, never modified: the fixture looks at its guards after every test that used it)."""
    rc, b = _routed(case)
    TOUCHED.append(b)
    return rc, b


@functools.lru_cache(maxsize=None)
def _routed(case):
    """The wire rows and the sorted order must be the stated ones."""
    rc = C.reduce_case(*case)
    rr = {'ids': rc['ids'], 'block': rc['n'], 'ent_off': rc['ent_off'], 'world': rc['world'], 'cap': rc['cap'], 'pair': rc['pair']}
    b = route(rr)
    out = check_routed(rr, b)
    lay = R.sort_layout(rc['n'], rc['W'])
    assert np.array_equal(out['inverse'], rc['inverse']) and np.array_equal(out['sort_ws'][lay['skey']:lay['skey'] + rc['m']], rc['skey'])
    rc['boundary'] = sorted(set(int(k) for k in R.predict_xkeys(rc['skey'], rc['m'], rc['n'], rc['d'], rc['opt']) if k >= 0))
    return rc, b


class chunk_option:
    """shard_chunk is process-wide: set for the block, always restored."""

    def __init__(self, opt):
        self.opt = opt

    def __enter__(self):
        self.old = lib().set_option('shard_chunk', self.opt)
        assert self.old == 0

    def __exit__(self, *exc):
        lib().set_option('shard_chunk', self.old)


def gwire_of(rc, fill, rng=None):
    g = np.full((rc['W'], rc['ld']), np.nan, np.float32)
    g[:, :rc['d']] = fill if rng is None else rng.standard_normal((rc['W'], rc['d'])).astype(np.float32)
    return g


def walk_args(rc, b, G, gw):
    return (G.ptr, rc['ld'], rc['d'], rc['n_src'], rc['src_off'], b['sort_ws'].ptr, rc['n'], rc['W'], gw.ptr, rc['ld'])


@pytest.mark.parametrize('case', CASES, ids=case_id)
def test_reduce_rows(case):
    """ktup_shard_reduce_rows ACCUMULATES onto a non-zero gwire: old + sum within k u (|old| + sum |terms|), a single-entry row
    exactly the one fp32 add, rows without entries and the NaN pitch columns bit-identical."""
    rc, b = routed(case)
    before = gwire_of(rc, 0, np.random.default_rng(C.seed_of('gwire', case)))
    G, gw = Buf(rc['G']), Buf(before)
    call('ktup_shard_reduce_rows', *walk_args(rc, b, G, gw), stream())
    ratio = R.check_reduced(gw.get(), before, rc['G'], rc['n_src'], rc['src_off'], rc['inverse'], rc['d'], False)
    assert np.array_equal(bits(G.get()), bits(rc['G']))
    print('%-28s reduce_rows %.3f' % (case_id(case), ratio))
    note('ktup_shard_reduce_rows', ratio)


@pytest.mark.parametrize('case', CASES, ids=case_id)
def test_reduce_store(case):
    """ktup_shard_zero_shared_rows + ktup_shard_reduce_store onto a NaN-filled gwire: rows without entries are still NaN (never
    written), single-entry rows bit-exact, shared rows within (k - 1) u sum |terms|."""
    rc, b = routed(case)
    before = gwire_of(rc, np.nan)
    G, gw = Buf(rc['G']), Buf(before)
    with chunk_option(rc['opt']):
        call('ktup_shard_zero_shared_rows', b['sort_ws'].ptr, rc['n'], rc['W'], b['inverse'].ptr, gw.ptr, rc['ld'], rc['d'], stream())
        call('ktup_shard_reduce_store', *walk_args(rc, b, G, gw), stream())
    ratio = R.check_reduced(gw.get(), before, rc['G'], rc['n_src'], rc['src_off'], rc['inverse'], rc['d'], True)
    print('%-28s reduce_store %.3f' % (case_id(case), ratio))
    note('ktup_shard_reduce_store', ratio)


def fold_bufs(rc, n_rep, second, rows=3):
    rng = np.random.default_rng(C.seed_of('fold', rc['d'], rc['name'], n_rep, second))
    elems = rows * rc['d']
    rep = rng.standard_normal((n_rep, 2, elems)).astype(np.float32)
    dst = [rng.standard_normal(elems).astype(np.float32) for _ in range(4 if second else 2)]
    return rep, dst, elems


def check_fold(rep, dst, got_rep, got_dst, n_rep):
    """dst[j] = old + sum of the replicas (A -> dst[0], dst[2]; C -> dst[1], dst[3]): one fp32 add for one replica (exact), n_rep
    roundings otherwise; the replicas are left +0.0."""
    assert not bits(got_rep).any(), 'the replicas must be left zero'
    worst = 0.0
    for j, old in enumerate(dst):
        part = rep[:, j % 2, :]
        if n_rep == 1:
            assert np.array_equal(got_dst[j], old + part[0])
            continue
        want = old.astype(np.float64) + part.astype(np.float64).sum(axis=0)
        tol = n_rep * R.U * (np.abs(old) + np.abs(part).sum(axis=0))
        err = np.abs(got_dst[j].astype(np.float64) - want)
        assert (err <= tol).all()
        worst = max(worst, float((err / tol).max()))
    return worst


@pytest.mark.parametrize('second', [False, True], ids=['gP_gPn', 'gP_gPn_gR_gRn'])
@pytest.mark.parametrize('n_rep', [1, 3])
@pytest.mark.parametrize('case', CASES, ids=case_id)
def test_reduce_store_fold(case, n_rep, second):
    """The store walk with the replica fold riding in extra workgroups: destinations get old + sum of the replicas, the replicas
    are left zero, gwire as ktup_shard_reduce_store."""
    rc, b = routed(case)
    before = gwire_of(rc, np.nan)
    rep, dst, elems = fold_bufs(rc, n_rep, second)
    G, gw, brep, bdst = Buf(rc['G']), Buf(before), Buf(rep), [Buf(x) for x in dst]
    with chunk_option(rc['opt']):
        call('ktup_shard_zero_shared_rows', b['sort_ws'].ptr, rc['n'], rc['W'], b['inverse'].ptr, gw.ptr, rc['ld'], rc['d'], stream())
        call('ktup_shard_reduce_store_fold', *walk_args(rc, b, G, gw), brep.ptr, n_rep, elems, ptrs(bdst + [None] * (4 - len(bdst))), stream())
    ratio = R.check_reduced(gw.get(), before, rc['G'], rc['n_src'], rc['src_off'], rc['inverse'], rc['d'], True)
    ratio = max(ratio, check_fold(rep, dst, brep.get(), [x.get() for x in bdst], n_rep))
    print('%-28s store_fold n_rep %d: %.3f of the tolerance' % (case_id(case), n_rep, ratio))
    note('ktup_shard_reduce_store_fold', ratio)


# (slots, dup_only, n_small, small_weight, fold, cursor)
NORM_OPTIONS = [(1, 0, 0, 1.0, False, False), (16, 0, 2, 2.0, True, True), (1, 1, 4, 1.0, True, False), (16, 1, 0, 1.0, False, True),
                (16, 0, 4, 1.0, False, False), (1, 1, 2, 2.0, False, True)]


def run_norm(rc, b, slots, dup, n_small, weight, fold, cursor, rep=None):
    """One ktup_shard_reduce_norm[_fold] launch on an all-zero gwire; returns everything it may write, downloaded."""
    d = rc['d']
    Gh = C.dup_only_G(rc) if dup else rc['G']                            # dup_only: NaN in the rows of entries alone on their row
    smalls = C.small_grads(rc, n_small)
    zero = gwire_of(rc, 0.0)
    n_list = R.list_len(rc['n'], d, rc['opt'])
    G, gw, xk = Buf(Gh), Buf(zero), Buf(np.full(n_list, -3, np.int32))
    sm = [Buf(s) for s in smalls]
    ss = Buf(np.full(slots + 2, 0.25))
    fd = Buf(np.asarray([1.5, -0.25, 3.0, 9.0])) if fold else None       # (the last one lies past n_fold = 3)
    cur = Buf(np.asarray([7, 41, 7], np.int64)) if cursor else None
    with chunk_option(rc['opt']):
        assert lib().load().ktup_shard_reduce_list_len(rc['n'], d) == n_list
        head = walk_args(rc, b, G, gw) + (xk.ptr, n_small, ptrs(sm), 3 * d, weight, ss.ptr + 8, slots, dup, fd.ptr if fold else None,
                                          3 if fold else 0, cur.ptr + 8 if cursor else None)
        if rep is None:
            call('ktup_shard_reduce_norm', *head, stream())
        else:
            brep, bdst, n_rep = rep
            call('ktup_shard_reduce_norm_fold', *head, brep.ptr, n_rep, ptrs(bdst + [None] * (4 - len(bdst))), stream())
    s = ss.get()
    assert s[0] == 0.25 and s[-1] == 0.25
    if fold:
        assert fd.get().tolist() == [0.0, 0.0, 0.0, 9.0], 'fold is added in and left zero'
    if cursor:
        assert cur.get().tolist() == [7, 42, 7], 'the cursor moves by exactly 1'
    for h, s0 in zip(sm, smalls):
        assert np.array_equal(bits(h.get()), bits(s0))
    assert np.array_equal(bits(G.get()), bits(Gh))
    return {'sumsq': s[1:-1] - 0.25, 'xkeys': xk.get(), 'gwire': gw.get(), 'smalls': smalls, 'G': Gh, 'fold': [1.5, -0.25, 3.0] if fold else None,
            'bufs': (G, gw, xk, sm, ss)}


def check_norm_outputs(rc, out, dup):
    """xkeys lists exactly the predicted boundary rows; gwire holds their sums and nothing else."""
    d = rc['d']
    want = R.predict_xkeys(rc['skey'], rc['m'], rc['n'], d, rc['opt'])
    R.check_xkeys(out['xkeys'], want)
    tot, mag, cnt = R.reduce_terms(out['G'], rc['n_src'], rc['src_off'], rc['inverse'], rc['W'], d)
    listed = np.zeros(rc['W'], bool)
    listed[rc['boundary']] = True
    gw = out['gwire']
    assert not bits(gw[~listed, :d]).any(), 'gwire holds something besides the boundary rows'
    assert np.isnan(gw[:, d:]).all()
    err = np.abs(gw[listed, :d].astype(np.float64) - tot[listed])
    tol = (cnt[listed, None] - 1) * R.U * mag[listed]
    assert (err <= tol).all(), 'a boundary row\'s sum'
    return float((err / tol).max()) if listed.any() else 0.0


@pytest.mark.parametrize('case', CASES, ids=case_id)
def test_reduce_norm(case):
    """ktup_shard_reduce_norm: 1 and 16 slots (the sum over slots is compared; several slots are used once several workgroups
    have entries), dup_only 0 / 1 (NaN planted where dup_only must not read), 0 / 2 / 4 small gradients at weight 1 and 2, fold
    added in and left zero, the cursor moved by exactly 1, xkeys and gwire exactly as the layout predicts."""
    rc, b = routed(case)
    for slots, dup, n_small, weight, fold, cursor in NORM_OPTIONS:
        out = run_norm(rc, b, slots, dup, n_small, weight, fold, cursor)
        want, tol = R.sumsq_ref(out['G'], rc['n_src'], rc['src_off'], rc['inverse'], rc['W'], rc['d'], rc['n'], dup, rc['boundary'],
                                out['smalls'], weight, out['fold'], rc['opt'])
        got = float(out['sumsq'].sum())
        ratio = R.check_sumsq(got, want, tol, (case, slots, dup))
        rows = check_norm_outputs(rc, out, dup)
        if slots == 16 and not dup and -(-rc['m'] // R.stretch(rc['n'], rc['d'], rc['opt'])) > 1:
            assert (out['sumsq'] != 0).sum() > 1, 'sixteen slots, one used'
        print('%-28s slots %2d dup_only %d small %d x %.0f: sumsq %.17g want %.17g  %.3f of the tolerance; boundary rows %.3f'
              % (case_id(case), slots, dup, n_small, weight, got, want, ratio, rows))
        note('ktup_shard_reduce_norm', ratio)


@pytest.mark.parametrize('second', [False, True], ids=['gP_gPn', 'gP_gPn_gR_gRn'])
@pytest.mark.parametrize('n_rep', [1, 3])
@pytest.mark.parametrize('case', CASES, ids=case_id)
def test_reduce_norm_fold(case, n_rep, second):
    """ktup_shard_reduce_norm_fold: the replicas are folded as by the store walk, and the norm's small-gradient term is that of the
    FOLDED values (weighted; every destination counts)."""
    rc, b = routed(case)
    rep, dst, elems = fold_bufs(rc, n_rep, second)
    assert elems == 3 * rc['d']
    brep, bdst = Buf(rep), [Buf(x) for x in dst]
    weight = 2.0
    out = run_norm(rc, b, 16, 0, 0, weight, True, True, rep=(brep, bdst, n_rep))
    got_dst = [x.get() for x in bdst]
    ratio = check_fold(rep, dst, brep.get(), got_dst, n_rep)
    folded = [old.astype(np.float64) + rep[:, j % 2, :].astype(np.float64).sum(axis=0) for j, old in enumerate(dst)]
    want, tol = R.sumsq_ref(out['G'], rc['n_src'], rc['src_off'], rc['inverse'], rc['W'], rc['d'], rc['n'], 0, rc['boundary'], (), 1.0,
                            out['fold'], rc['opt'])
    # a thread folds and squares at most ks elements of each destination pair: ks = ceil(2 elems / (blocks x 256)) fmas, as the small
    # gradients' bound; the folded value itself carries n_rep roundings: d(v^2) = 2 |v| n_rep u (|old| + sum |replicas|)
    blocks = -(-2 * elems // 256)
    ks = 2 * -(-2 * elems // (blocks * 256))
    for j, v in enumerate(folded):
        mag = np.abs(dst[j]).astype(np.float64) + np.abs(rep[:, j % 2, :]).astype(np.float64).sum(axis=0)
        want += weight * float((v ** 2).sum())
        tol += weight * R.U * ((3 * ks + 9) * float((v ** 2).sum()) + float((2 * np.abs(v) * n_rep * mag).sum()))
    ratio = max(ratio, R.check_sumsq(float(out['sumsq'].sum()), want, tol, (case, n_rep, second)))
    check_norm_outputs(rc, out, 0)
    print('%-28s norm_fold n_rep %d: %.3f of the tolerance' % (case_id(case), n_rep, ratio))
    note('ktup_shard_reduce_norm_fold', ratio)


# ------------------------------------------------------------------------------------------------ apply
APPLY_OPTIONS = C.APPLY_OPTIONS                                       # (kind, clip, skip, n_small, second summand table, small_g64, slots, stale)


class Step:
    """The device side of an apply case: tables, states, small tables, the books; the argument tail both apply forms share."""

    def __init__(self, c):
        self.c = c
        self.tables = [Buf(P) for P in c['tables']]
        self.states = [Buf(S) for S in c['states']] if c['states'] is not None else None
        self.ids = Buf(c['ids'])
        sm = c['smalls']
        self.sg = [Buf(s['g']) for s in sm]
        self.sp0 = [Buf(s['p0']) for s in sm]
        self.ss0 = [Buf(s['s0']) if s['s0'] is not None else None for s in sm]
        self.sp1 = [Buf(s['p1']) if s['p1'] is not None else None for s in sm]
        self.ss1 = [Buf(s['s1']) if s['s1'] is not None else None for s in sm]
        g64 = [s['g64'] for s in sm if s['g64'] is not None]
        self.g64 = Buf(np.stack(g64)) if g64 else None
        self.skip_i = Buf(np.asarray([0, c['skip_count'], 0], np.int32))
        self.skip_d = Buf(np.asarray([0.0, c['skip_value'], 0.0]))
        self.loss_step, self.loss_sum = Buf(c['loss_step']), Buf(c['loss_sum'])
        self.skipped = Buf(np.asarray([3, c['skipped'], 3], np.int32))
        self.step = Buf(np.asarray([-1, c['t'] - 1, 0, -1], np.int64))
        self.rule = None
        if c['kind'] == R.ADAM:
            self.rule = AdamRule(c['beta1'], c['beta2'], c['replay'], c['rule'], self.step.ptr + 8, c['wd'], 0.0)

    def count(self):
        """ktup_shard_step_count: the launch before the apply launch (+1 unless skipped, the bias corrections refreshed)."""
        c = self.c
        call('ktup_shard_step_count', self.step.ptr + 8, self.skip_i.ptr + 4, self.skip_d.ptr + 8, c['beta1'], c['beta2'], stream())

    def head(self):
        c = self.c
        return (c['kind'], c['T'], ptrs(self.tables), i64(P.shape[1] for P in c['tables']), ptrs(self.states) if self.states else None,
                i64(S.shape[1] for S in c['states']) if self.states else None, i64(c['cap']))

    def tail(self, sumsq):
        c = self.c
        n_small = len(c['smalls'])
        any1 = any(h is not None for h in self.sp1)
        return (n_small, 3, ptrs(self.sg), ptrs(self.sp0), ptrs(self.ss0) if c['kind'] != R.SGD else None, ptrs(self.sp1) if any1 else None,
                ptrs(self.ss1) if any1 and c['kind'] != R.SGD else None, self.g64.ptr if self.g64 else None, c['lr'], c['eps'],
                sumsq.ptr + 8, c['slots'], c['max_norm'], self.skip_i.ptr + 4, self.skip_d.ptr + 8, self.loss_step.ptr, c['n_loss'],
                self.loss_sum.ptr, self.skipped.ptr + 4, ctypes.addressof(self.rule) if self.rule else None, stream())

    def download(self, grads, before, zero_mask):
        c = self.c
        got = {'tables': [h.get() for h in self.tables], 'states': [h.get() for h in self.states] if self.states else [], 'small': []}
        for k in range(len(c['smalls'])):
            got['small'].append({'g': self.sg[k].get(), 'p0': self.sp0[k].get(), 's0': self.ss0[k].get() if self.ss0[k] else None,
                                 'p1': self.sp1[k].get() if self.sp1[k] else None, 's1': self.ss1[k].get() if self.ss1[k] else None})
        d = c['d']
        got['grads'], got['grads_before'], got['grads_zero'] = grads[:, :d], before[:, :d], zero_mask
        assert np.array_equal(bits(grads[:, d:]), bits(before[:, d:])), 'pitch columns of the gradient buffer'
        got['loss_step'], got['loss_sum'] = self.loss_step.get(), self.loss_sum.get()
        sk = self.skipped.get()
        assert sk[0] == 3 and sk[2] == 3
        got['skipped'] = sk[1]
        skip = bool(c['skip_count']) or c['skip_value'] != 0.0
        st = self.step.get()
        assert st[0] == -1 and st[3] == -1
        if c['kind'] == R.ADAM:
            assert st[1] == (c['t'] - 1 if skip else c['t']), 'the step counter moves by one unless the step is skipped'
        assert np.array_equal(self.ids.get(), c['ids'])
        assert self.skip_i.get().tolist() == [0, c['skip_count'], 0] and self.skip_d.get().tolist() == [0.0, c['skip_value'], 0.0]
        if self.g64:
            assert np.array_equal(self.g64.get(), np.stack([s['g64'] for s in c['smalls']]))
        return got


def small_weight_of(c):
    return 2.0 if any(s['p1'] is not None for s in c['smalls']) else 1.0


def small_sq(c):
    """What the clip norm holds for the small gradients: the local fp32 ones (the fp64 bucket only replaces the VALUES stepped with)."""
    return small_weight_of(c) * sum(float((s['g'].astype(np.float64) ** 2).sum()) for s in c['smalls'])


@pytest.mark.parametrize('case', CASES, ids=case_id)
def test_reduce_apply(case):
    """norm -> step_count -> ktup_shard_reduce_apply for SGD, Adagrad, Adam and the two weight-decay rules: max_norm that clips, one
    that does not, 0 and negative; rows with ids[w] = -1 untouched (one of them a LISTED boundary row, whose sum must still leave
    gwire; rows with entries and rows without); small tables with and
    without the second summand table and with small_g64; skip_count / skip_value; the loss slots; touched rows that owe 1, 3 and 6
    steps (stale: Adam's replay, rules 0 / 1 / 2 under weight decay) beside two stale rows no entry names.  gwire all-zero afterwards;
    every element of every buffer compared."""
    rc, b = routed(case)
    d = rc['d']
    for kind, clip, skip, n_small, second, g64, slots, stale in APPLY_OPTIONS:
        c = C.apply_case(rc, kind, clip=clip, skip=skip, n_small=n_small, second=second, g64=g64, slots=slots, boundary=rc['boundary'], stale=stale)
        weight = small_weight_of(c)
        st = Step(c)
        zero = gwire_of(rc, 0.0)
        G, gw, xk = Buf(rc['G']), Buf(zero), Buf(np.full(R.list_len(rc['n'], d, rc['opt']), -3, np.int32))
        ss = Buf(np.zeros(slots + 2))
        with chunk_option(rc['opt']):
            call('ktup_shard_reduce_norm', *walk_args(rc, b, G, gw), xk.ptr, n_small, ptrs(st.sg), 3 * d, weight, ss.ptr + 8, slots, 0,
                 None, 0, None, stream())
            sumsq = float(ss.get()[1:-1].sum())
            want, tol = R.sumsq_ref(rc['G'], rc['n_src'], rc['src_off'], rc['inverse'], rc['W'], d, rc['n'], 0, rc['boundary'],
                                    [s['g'] for s in c['smalls']], weight, None, rc['opt'])
            R.check_sumsq(sumsq, want, tol)
            c['max_norm'] = C.max_norm_of(clip, want)
            st.count()
            call('ktup_shard_reduce_apply', *st.head(), st.ids.ptr, rc['world'], G.ptr, rc['ld'], d, rc['n_src'], rc['src_off'],
                 b['sort_ws'].ptr, rc['n'], gw.ptr, rc['ld'], xk.ptr, *st.tail(ss))
        gsum, mag, cnt = R.reduce_terms(rc['G'], rc['n_src'], rc['src_off'], rc['inverse'], rc['W'], d)
        delta = np.maximum(cnt - 1, 0)[:, None] * R.U * mag
        ref = R.apply_ref(c, gsum, delta, (c['ids'] >= 0) & (cnt > 0), want, tol)
        got = st.download(gw.get(), zero, np.ones((rc['W'], d), bool))
        ratio = R.check_apply(c, ref, got)
        assert ss.get()[0] == 0 and ss.get()[-1] == 0
        print('%-28s %-10s clip %-8s skip %-5s stale %d: coef %.4f  %.3f of the tolerance' % (case_id(case), kind, clip, skip, stale, ref['coef'], ratio))
        note('ktup_shard_reduce_apply', ratio)


@pytest.mark.parametrize('case', CASES, ids=case_id)
def test_apply(case):
    """ktup_shard_apply, the gradient-buffer form, on the same cases: every wire row with ids[w] >= 0 is stepped with its row of the
    buffer (the fp32 reduction of the case; the squared norm is handed in as doubles), consumed rows are zero-filled, rows with
    ids[w] < 0 keep their gradient."""
    rc, b = routed(case)
    d, W = rc['d'], rc['W']
    for kind, clip, skip, n_small, second, g64, slots, stale in APPLY_OPTIONS:
        c = C.apply_case(rc, kind, clip=clip, skip=skip, n_small=n_small, second=second, g64=g64, slots=slots, boundary=rc['boundary'], stale=stale)
        st = Step(c)
        before = gwire_of(rc, 0.0)
        before[:, :d] = R.emulate_reduce(rc['G'], rc['n_src'], rc['src_off'], rc['inverse'], W, d)
        gsum = before[:, :d].astype(np.float64)
        sumsq = float((gsum ** 2).sum()) + small_sq(c)
        c['max_norm'] = C.max_norm_of(clip, sumsq)
        parts = np.zeros(slots + 2)
        parts[1:-1] = sumsq / slots
        ss, grads = Buf(parts), Buf(before)
        st.count()
        call('ktup_shard_apply', *st.head(), d, st.ids.ptr, rc['world'], grads.ptr, rc['ld'], *st.tail(ss))
        ref = R.apply_ref(c, gsum, np.zeros_like(gsum), c['ids'] >= 0, float(parts[1:-1].sum()), 0.0)
        zero_mask = np.repeat((c['ids'] >= 0)[:, None], d, axis=1)
        ratio = R.check_apply(c, ref, st.download(grads.get(), before, zero_mask))
        print('%-28s %-10s clip %-8s skip %-5s stale %d: coef %.4f  %.3f of the tolerance' % (case_id(case), kind, clip, skip, stale, ref['coef'], ratio))
        note('ktup_shard_apply', ratio)


@pytest.mark.parametrize('case', [c for c in CASES if c[1] in ('padded', 'ktup')] + [(6, 'padded', 0, False)], ids=case_id)
def test_pack_wire(case):
    """out[w] = table_t[ids[w]] bit for bit; rows with ids[w] < 0 and the pitch columns keep their NaN prefill (d = 6: scalar rows)."""
    if case[0] == 6:
        rc = C.reduce_case(4, 'padded')
        rc = dict(rc, d=6, ld=6, boundary=[])
    else:
        rc, _ = routed(case)
    d, W, T = rc['d'], rc['W'], rc['T']
    c = C.apply_case(rc, 'sgd', boundary=rc['boundary'])
    tables = [Buf(P) for P in c['tables']]
    ids, out = Buf(c['ids']), Buf(np.full((W, rc['ld']), np.nan, np.float32))
    call('ktup_shard_pack_wire', T, ptrs(tables), i64(P.shape[1] for P in c['tables']), i64(rc['cap']), d, ids.ptr, rc['world'], out.ptr,
         rc['ld'], stream())
    got = out.get()
    want = np.full((W, rc['ld']), np.nan, np.float32)
    for w in np.nonzero(c['ids'] >= 0)[0]:
        want[w, :d] = c['tables'][w % T][c['ids'][w], :d]
    assert np.array_equal(bits(got), bits(want))
    for h, P in zip(tables, c['tables']):
        assert np.array_equal(bits(h.get()), bits(P))


# ------------------------------------------------------------------------------------------------ refusals
def test_refusals():
    """By status and message only: d = 1028 and d = 6 for the fused walks, a pitch that is no multiple of 4, a gwire that is not
    16-byte aligned, a phase outside 0 .. 5, pair_map over unequal tables, n_entries % block != 0, world = 65.  Nothing is
    launched: the buffers (large enough for the refused shape anyway) and their guards come back untouched."""
    rc, b = routed((64, 'm_S_p1', 0, False))
    n, W = rc['n'], rc['W']
    Gh, gh = np.full((n, 1032), 1.0, np.float32), np.full((W, 1032), 2.0, np.float32)
    G, gw, xk, ss = Buf(Gh), Buf(gh), Buf(np.full(2 * n, -3, np.int32)), Buf(np.zeros(3))

    def walks(d, ld, gptr):
        head = (G.ptr, ld, d, n, 0, b['sort_ws'].ptr, n, W, gptr, ld)
        return [('ktup_shard_reduce_store', head + (stream(),)),
                ('ktup_shard_reduce_norm', head + (xk.ptr, 0, None, 0, 1.0, ss.ptr + 8, 1, 0, None, 0, None, stream()))]
    for d, ld, gptr, word in ((1028, 1028, gw.ptr, 'd % 4'), (6, 8, gw.ptr, 'd % 4'), (64, 66, gw.ptr, '16-byte'), (64, 64, gw.ptr + 4, '16-byte')):
        for name, args in walks(d, ld, gptr):
            rc_, msg = refused(name, *args)
            assert rc_ == lib().ERR_UNSUPPORTED and word in msg and name[:17] in msg, (name, d, rc_, msg)
    tab = Buf(np.zeros((70, 1032), np.float32))
    ids = Buf(np.full(W, -1, np.int64))
    for d in (1028, 6):
        rc_, msg = refused('ktup_shard_reduce_apply', R.SGD, rc['T'], ptrs([tab] * rc['T']), i64([1032] * rc['T']), None, None, i64(rc['cap']),
                           ids.ptr, rc['world'], G.ptr, 1032, d, n, 0, b['sort_ws'].ptr, n, gw.ptr, 1032, xk.ptr, 0, 0, None, None, None,
                           None, None, None, 0.05, 1e-6, ss.ptr + 8, 1, 0.0, None, None, None, 0, None, None, None, stream())
        assert rc_ == lib().ERR_UNSUPPORTED and 'd % 4' in msg, (d, rc_, msg)
    assert lib().load().ktup_shard_reduce_list_len(n, 6) == 0
    kb = C.ktup_batches()
    rr = _ktup_rc(kb, 0)
    kbuf = _ktup_route(kb, 0, ())
    B = kb['B']
    for phase in (-1, 6):
        rc_, msg = refused('ktup_shard_route_ktup', kbuf['u'].ptr, kbuf['pos'].ptr, kbuf['neg'].ptr, B, kb['n_batches'], kbuf['cursor'].ptr + 8,
                           kbuf['item2ent'].ptr, kb['ent_pad'], kbuf['ids'].ptr, kb['world'], i64(kb['cap']), kbuf['inverse'].ptr,
                           kbuf['send_ids'].ptr, kbuf['pair_map'].ptr, kbuf['sort_ws'].ptr, kbuf['counters'].ptr, kbuf['zero'].ptr, 3,
                           kbuf['ws'].ptr, phase, stream())
        assert rc_ != 0 and 'phase' in msg, (phase, rc_, msg)

    def plain(block, ent_off, world, pair_map):
        return refused('ktup_shard_route', kbuf['ids'].ptr, len(rr['ids']), block, 3, i64(ent_off), world, i64(kb['cap']), 1, 2,
                       kbuf['inverse'].ptr, kbuf['send_ids'].ptr, pair_map, kbuf['sort_ws'].ptr, kbuf['counters'].ptr, None, 0,
                       kbuf['ws'].ptr, stream())
    for args, word in (((5 * B, [0, B, 3 * B - 1, 5 * B], kb['world'], kbuf['pair_map'].ptr), 'pair_map'),
                       ((5 * B - 1, [0, B, 3 * B, 5 * B - 1], kb['world'], None), 'block'),
                       ((5 * B, [0, B, 3 * B, 5 * B], 65, None), '64 ranks')):
        rc_, msg = plain(*args)
        assert rc_ != 0 and word in msg, (word, rc_, msg)
    for h, want in ((G, Gh), (gw, gh)):
        assert np.array_equal(h.get(), want)
    for k in ROUTE_KEYS:
        if kbuf[k] is not None:
            kbuf[k].get()                                                 # (guards)
    assert (kbuf['ids'].get() == -11).all() and (xk.get() == -3).all() and not ss.get().any()


# ------------------------------------------------------------------------------------------------ the small calls
@pytest.mark.parametrize('slots', [1, 16])
@pytest.mark.parametrize('n_small', [0, 1, 4])
def test_bucket(n_small, slots):
    """mode 0: bucket = [small gradients as doubles | the sum of the slots | the overflow word as a double]; mode 1: *sumsq_total =
    bucket[N] + small_weight x sum of squares of bucket[0 .. N) -- doubles throughout: exact conversions, sums to N x 2^-53."""
    rng = np.random.default_rng(C.seed_of('bucket', n_small, slots))
    elems = 3 * 100
    sg = [rng.standard_normal(elems).astype(np.float32) for _ in range(n_small)]
    N = n_small * elems
    local = rng.random(slots + 2)
    hs, hl, ov = [Buf(s) for s in sg], Buf(local), Buf(np.asarray([0, 12345, 0], np.int32))
    bucket, total = Buf(np.full(N + 4, np.nan)), Buf(np.full(3, np.nan))
    call('ktup_shard_bucket', 0, n_small, ptrs(hs), elems, bucket.ptr + 8, hl.ptr + 8, slots, ov.ptr + 4, None, 1.0, stream())
    got = bucket.get()
    assert np.isnan(got[0]) and np.isnan(got[-1])
    flat = np.concatenate(sg).astype(np.float64) if n_small else np.zeros(0)
    assert np.array_equal(got[1:N + 1], flat) and got[N + 2] == 12345.0
    want = float(local[1:-1].sum())
    assert abs(got[N + 1] - want) <= slots * 2.0 ** -53 * want
    for weight in (1.0, 2.0):
        call('ktup_shard_bucket', 1, n_small, None, elems, bucket.ptr + 8, None, 0, None, total.ptr + 8, weight, stream())
        t = total.get()
        sq = float((flat ** 2).sum())
        assert np.isnan(t[0]) and np.isnan(t[2]) and abs(t[1] - (got[N + 1] + weight * sq)) <= (N + 2) * 2.0 ** -53 * (got[N + 1] + weight * sq)
    assert np.array_equal(bits(bucket.get()[1:-1]), bits(got[1:-1]))


@pytest.mark.parametrize('t', [1, 10, 1000, 100000])
def test_step_count(t):
    """The counter moves by one unless skip_count or skip_value is non-zero; step[1] = {1 - beta1^t, sqrt(1 - beta2^t)} as two floats:
    the device evaluates pow / sqrt in double (a few ulps of a double) and rounds to float, so at most ONE float ulp from the fp64 value
    rounded here."""
    b1, b2 = float(np.float32(0.9)), float(np.float32(0.999))
    for skip_i, skip_d in ((0, 0.0), (1, 0.0), (0, -0.5)):
        step = Buf(np.asarray([-1, t - 1, 0x1234567812345678, -1], np.int64))
        si, sd = Buf(np.asarray([skip_i], np.int32)), Buf(np.asarray([skip_d]))
        call('ktup_shard_step_count', step.ptr + 8, si.ptr, sd.ptr, b1, b2, stream())
        got = step.get()
        if skip_i or skip_d:
            assert got.tolist() == [-1, t - 1, 0x1234567812345678, -1]
            continue
        assert got[0] == -1 and got[1] == t and got[3] == -1
        bc = got[2:3].view(np.float32)
        want = np.asarray([1.0 - b1 ** t, np.sqrt(1.0 - b2 ** t)]).astype(np.float32)
        ulps = np.abs(bc.view(np.int32).astype(np.int64) - want.view(np.int32).astype(np.int64))
        print('t %6d: bias corrections %r want %r (%s ulp)' % (t, bc.tolist(), want.tolist(), ulps.tolist()))
        assert (ulps <= 1).all()
    step = Buf(np.asarray([t - 1, 0], np.int64))
    call('ktup_shard_step_count', step.ptr, None, None, b1, b2, stream())           # both flags may be NULL
    assert step.get()[0] == t


@pytest.mark.parametrize('form', ['ids_null', 'some_null', 'lists'])
@pytest.mark.parametrize('n_seg', [1, 3, 8])
@pytest.mark.parametrize('gap', C.CATCHUP_GAPS)
@pytest.mark.parametrize('rule,wd', [(0, 0.0), (0, 1e-2), (1, 1e-2), (2, 1e-2)], ids=['adam', 'adam_wd', 'adagrad_wd', 'sgd_wd'])
def test_adam_catchup(rule, wd, gap, n_seg, form):
    """ktup_shard_adam_catchup over 1, 3 and 8 segments, with ids == NULL, some ids[k] == NULL and id lists with padding: listed rows
    written at an earlier step are replayed to *step (stamp = *step), rows never written, rows already at *step and rows not listed
    come back bit for bit.  Against the fp64 recurrence of the flush test at 4 x the fp32 emulation's error, measured by
    tests/test_shard_ref_host.py::test_adam_replay_fp32_error_is_the_tolerance: gap 3 (replays of 3 .. 61 steps, the step-by-step
    and the series form): p 1.34e-06 absolute, m 6.7e-07 and v 8.15e-07 relative; gap 20 (20 .. 78 steps, the series form): p 1.30e-06,
    m 7.95e-07, v 8.0e-07.  On the GPU the launch uses 0.23 (gap 3) and 0.18 (gap 20) of four times that, at most 0.27 under weight decay.
    Under weight decay (rule 0 Adam, 1 Adagrad, 2 SGD; include/ktup_hip.h "WEIGHT DECAY") every listed row owes its steps on g = wd * p,
    one by one: the reference is tests/_shard_ref.lazy_rows (pinned to dense torch.optim on the CPU), the tolerance again 4 x the fp32
    emulation's error; an array the rule does not write (m for rules 1 and 2, v for rule 2) comes back bit for bit."""
    c = C.catchup_case(gap, rule=rule, wd=wd)
    d, n = c['d'], c['n']
    tol = R.replay_tolerance(c)
    want_p, want_m, want_v = R.replay_expected(c)
    rng = np.random.default_rng(C.seed_of('catchup_ids', gap, n_seg, form))
    tabs, sts, lists, n_rows = [], [], [], []
    for k in range(n_seg):
        tabs.append(Buf(c['p']))
        sts.append(Buf(c['S']))
        if form == 'ids_null' or (form == 'some_null' and k % 2 == 0):
            lists.append(None)
            n_rows.append(n - k)                                          # rows 0 .. n_rows - 1
        else:
            rows = rng.permutation(n)[:n // 2 + k].astype(np.int64)
            rows[k::5] = -1                                               # padding
            lists.append(rows)
            n_rows.append(len(rows))
    hl = [Buf(x) if x is not None else None for x in lists]
    step = Buf(np.asarray([c['t'], 0], np.int64))
    ar = AdamRule(c['beta1'], c['beta2'], c['replay'], c['rule'], step.ptr, c['wd'], 0.0)
    call('ktup_shard_adam_catchup', n_seg, ptrs(tabs), i64([d] * n_seg), ptrs(sts), i64([R.adam_pitch(d)] * n_seg),
         None if form == 'ids_null' else ptrs(hl), i64(n_rows), d, c['lr'], c['eps'], ctypes.addressof(ar), stream())
    worst = 0.0
    for k in range(n_seg):
        listed = np.zeros(n, bool)
        listed[np.arange(n_rows[k]) if lists[k] is None else lists[k][lists[k] >= 0]] = True
        moved = listed & (c['last'] < c['t']) & ((c['last'] > 0) | (c['wd'] > 0))
        P, S = tabs[k].get(), sts[k].get()
        assert np.array_equal(bits(P[~moved]), bits(c['p'][~moved])) and np.array_equal(bits(S[~moved]), bits(c['S'][~moved]))
        assert (S[moved, 2 * d].view(np.int32) == c['t']).all() and np.array_equal(bits(S[:, 2 * d + 1:]), bits(c['S'][:, 2 * d + 1:]))
        ratios = []
        for key, got, before, want in (('p', P, c['p'], want_p), ('m', S[:, :d], c['S'][:, :d], want_m), ('v', S[:, d:2 * d], c['S'][:, d:2 * d], want_v)):
            if not tol[key][moved].any():                                 # the rule does not write this array
                assert np.array_equal(bits(got[moved]), bits(before[moved])), key
            else:
                ratios.append(float((np.abs(got[moved].astype(np.float64) - want[moved]) / tol[key][moved]).max()))
        worst = max([worst] + ratios)
        assert all(r <= 1.0 for r in ratios), (k, ratios)
    print('rule %d wd %g gap %2d %d segments %-9s: %.3f of 4 x the fp32 replay error' % (rule, wd, gap, n_seg, form, worst))
    note('ktup_shard_adam_catchup', worst)


@pytest.mark.parametrize('nbytes', [0, 16, 16 * 4097])
def test_zero_async(nbytes):
    """Zero-fill by a kernel: 0, 16 and 16 x 4097 bytes inside guards; a misaligned pointer and a size that is no multiple of 16 are refused."""
    h = Buf(np.full(nbytes + 32, 0xEE, np.uint8))
    call('ktup_zero_async', h.ptr + 16 if nbytes else None, nbytes, stream())
    got = h.get()
    assert (got[:16] == 0xEE).all() and (got[16 + nbytes:] == 0xEE).all() and not got[16:16 + nbytes].any()
    for ptr, size in ((h.ptr + 4, 16), (h.ptr, 24)):
        rc_, msg = refused('ktup_zero_async', ptr, size, stream())
        assert rc_ != 0 and '16-byte' in msg
    assert np.array_equal(h.get(), got)


ENTRY_POINTS = ('ktup_shard_route', 'ktup_shard_route_ktup', 'ktup_shard_route_kg', 'ktup_shard_ktup_entries', 'ktup_shard_pack_wire',
                'ktup_shard_reduce_rows', 'ktup_shard_reduce_store', 'ktup_shard_reduce_store_fold', 'ktup_shard_reduce_norm',
                'ktup_shard_reduce_norm_fold', 'ktup_shard_reduce_apply', 'ktup_shard_zero_shared_rows', 'ktup_shard_apply',
                'ktup_shard_bucket', 'ktup_shard_step_count', 'ktup_shard_adam_catchup', 'ktup_zero_async')


def test_every_entry_point_is_launched_by_this_module():
    """Static: every public entry point of the sharded step appears as the name of a call() in this file's source."""
    import inspect
    import sys
    src = inspect.getsource(sys.modules[__name__])
    missing = [name for name in ENTRY_POINTS if "call('%s'" % name not in src]
    assert not missing, missing


def test_zz_report():
    """Prints the largest error / tolerance per entry point over whatever part of the module ran (each case asserts its own)."""
    for name in sorted(WORST):
        print('%-32s largest error / tolerance %.3f' % (name, WORST[name]))
        assert WORST[name] <= 1.0
