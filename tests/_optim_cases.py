"""The cases of tests/test_hip_optim_abi.py: shapes, hyper-parameter variants and one builder per test family, each a call of
tests/_optim_ref.case with a seed derived from the case's own name.  Host-only and deterministic, so tests/test_optim_ref_host.py
can build every case on the CPU and assert the generator's promises without a GPU.  NOT a test module."""
import zlib

from tests import _optim_ref as R

# (kind, momentum, first)
VARIANTS = [(R.SGD, 0.0, 0), (R.SGD, 0.9, 0), (R.SGD, 0.9, 1), (R.ADAGRAD, 0.0, 0), (R.ADAM, 0.0, 0),
            (R.RMSPROP, 0.0, 0), (R.RMSPROP, 0.9, 0), (R.RMSPROP, 0.9, 1)]
FOUR = [(R.SGD, 0.9, 0), (R.ADAGRAD, 0.0, 0), (R.ADAM, 0.0, 0), (R.RMSPROP, 0.9, 0)]     # one form of every kind, all state in use


def vid(v):
    return '%s-m%g-f%d' % (R.KIND_NAMES[v[0]], v[1], v[2])


def seed_of(*parts):
    return zlib.crc32(repr(parts).encode())


def build(family, key, variant, sizes, **kw):
    kind, momentum, first = variant
    return R.case(kind, sizes, seed_of(family, key, variant), momentum=momentum, first=first, family=family, **kw)


# ------------------------------------------------------------------------------------------------ the cases
SINGLES = (1, 3, 4, 5, 1023, 1024, 1025, 4093, 4095, 4096, 4097, 8191)
LISTS = {'odd_then_more': [5, 1023, 4097, 3, 8], 'empty_first': [0, 5, 4096], 'empty_middle': [7, 0, 4097],
         'empty_last': [1025, 6, 0], 'twelve_mixed': list(SINGLES), 'twelve_ones': [1] * 12}
SHAPES = dict([('n%d' % n, [n]) for n in SINGLES], **LISTS)
HYPER_SIZES = [4097, 5, 1023]
GRID_LABELS = ('4', '28', '32', '36', '68', 'cap-4', 'cap', 'resident', 'resident+4')


def sizes_for_chunks(ch):
    """A list of `ch` chunks with tails and a seam inside."""
    if ch == 1:
        return [4093]
    if ch == 2:
        return [4097]
    return [(ch - 2) * R.CHUNK - 3, 5, 4095]


def grid_chunks(label, cap):
    """Chunks of the list behind a grid label; a unit is a quarter chunk, so the boundaries need a capacity that is a multiple of 4."""
    assert cap >= 8 and cap % 4 == 0, cap
    table = {'cap-4': cap - 4, 'cap': cap, 'resident': R.CS_UPT * cap, 'resident+4': R.CS_UPT * cap + 4}
    units = table[label] if label in table else int(label)
    assert units >= 4 and units % 4 == 0
    return units // 4


def tails_case(shape, variant):
    return build('tails', shape, variant, SHAPES[shape], wd=1e-5, clip='below')


def tail_weight_case(variant):
    return build('tail_weight', 0, variant, [4099], wd=1e-5, clip='below', heavy_tail=True)


def hyper_case(variant, wd, clip):
    return build('hyper', (wd, clip), variant, HYPER_SIZES, wd=wd, clip=clip)


def zero_case(variant, zero_state):
    return build('zero', zero_state, variant, HYPER_SIZES, wd=0.0, clip='unit', zero_grad=True, zero_state=zero_state)


def zero_grads_case(variant, clip):
    return build('zero_grads', clip, variant, HYPER_SIZES, wd=1e-5, clip=clip, zero_grads=1)


def grid_case(label, variant, cap):
    return build('grids', label, variant, sizes_for_chunks(grid_chunks(label, cap)), wd=1e-5, clip='below')


REUSE = (('4', FOUR[2]), ('cap', FOUR[0]), ('36', FOUR[3]), ('resident+4', FOUR[1]), ('4', FOUR[2]))


def reuse_case(i, cap):
    label, variant = REUSE[i]
    return build('reuse', i, variant, sizes_for_chunks(grid_chunks(label, cap)), wd=1e-5, clip='below', zero_grads=i % 2)


STRIDE = {'step_2049': (FOUR[0], [2047 * R.CHUNK + 1, 5]), 'gradnorm_257': (FOUR[1], [255 * R.CHUNK + 3, 7])}


def stride_case(name):
    variant, sizes = STRIDE[name]
    assert R.n_chunks(sizes) == int(name.split('_')[1])
    return build('stride', name, variant, sizes, wd=1e-5, clip='below')


ACC_SIZES = {'small': [4097, 5, 40000], 'chunks_1025': [1023 * R.CHUNK + 1, 4097]}


def acc_case(name):
    return build('acc', name, FOUR[0], ACC_SIZES[name], clip='off')


def adam_case():
    return build('adam_steps', 0, FOUR[2], HYPER_SIZES, wd=1e-5, clip='below', steps=[1, 7, 100000])


def gnorm_case(variant, zero_grads):
    return build('gnorm', zero_grads, variant, HYPER_SIZES, wd=1e-5, clip='below', zero_grads=zero_grads)


def loss_case(clip):
    return build('loss', clip, FOUR[2], [4097, 5], wd=1e-5, clip=clip)


def graph_case():
    return build('graph', 0, FOUR[2], HYPER_SIZES, wd=1e-5, clip='unit', steps=[1, 7, 100000])


def refused_case(variant, n=3):
    return build('refused', n, variant, [8] * n, wd=1e-5, clip='below')


def all_case_builders(cap, cap_only=False):
    """Every case of this module as a thunk (tests/test_optim_ref_host.py builds them all on the CPU)."""
    out = []
    out += [lambda g=g, v=v: grid_case(g, v, cap) for g in GRID_LABELS for v in FOUR]
    out += [lambda i=i: reuse_case(i, cap) for i in range(len(REUSE))]
    if cap_only:
        return out
    out += [lambda s=s, v=v: tails_case(s, v) for s in SHAPES for v in FOUR]
    out += [lambda v=v: tail_weight_case(v) for v in FOUR]
    out += [lambda v=v, w=w, c=c: hyper_case(v, w, c) for v in VARIANTS for w in (0.0, 1e-5, 0.1) for c in ('off', 'unit', 'below')]
    out += [lambda v=v, z=z: zero_case(v, z) for v in VARIANTS for z in (False, True)]
    out += [lambda v=v, c=c: zero_grads_case(v, c) for v in FOUR for c in ('off', 'below')]
    out += [lambda n=n: stride_case(n) for n in STRIDE] + [lambda n=n: acc_case(n) for n in ACC_SIZES]
    out += [adam_case, graph_case] + [lambda v=v, z=z: gnorm_case(v, z) for v in FOUR for z in (0, 1)]
    out += [lambda c=c: loss_case(c) for c in ('off', 'below')] + [lambda v=v: refused_case(v) for v in VARIANTS]
    out += [lambda: refused_case(FOUR[2], 13)]
    return out
