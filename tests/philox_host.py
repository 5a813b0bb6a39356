"""Host model of the library's Philox4x32-10 streams (include/ktup_hip.h; csrc/ktup_common.h struct Philox), in vectorised numpy.

A stream is (seed, tag): the key is the two 32-bit halves of `seed`, the counter of block b is (b lo, b hi, tag lo, tag hi), and
draw i of the stream is word i & 3 of block i >> 2 -- positions are 64-bit, so a block index beyond 2^32 carries into the second
counter word.  Two tags are in use: GATE_TAG for the ST-Gumbel gate's uniforms and SAMPLER_TAG for the negative samplers.

Nothing here imports the library: the round function is checked against the published known-answer vectors on the CPU
(tests/test_philox_host.py), and the device kernels are then compared with this model."""
import numpy as np

GATE_TAG = 0x4b545550       # "KTUP": the preference gate's noise
SAMPLER_TAG = 0x4e454753    # "NEGS": ktup_negsample_* / ktup_feed_*

_M32 = np.uint64(0xffffffff)
_S32 = np.uint64(32)
_MUL0, _MUL1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
_W0, _W1 = np.uint64(0x9E3779B9), np.uint64(0xBB67AE85)


def philox4x32_10(counter, key):
    """The raw round function: counter = four arrays (or scalars) of 32-bit words, key = two -> four uint64 arrays holding the
    32-bit output words (Salmon et al., SC'11; Random123's philox4x32 with 10 rounds)."""
    c = [np.atleast_1d(np.asarray(x, dtype=np.uint64)) & _M32 for x in counter]
    c = list(np.broadcast_arrays(*c))
    a, b = np.uint64(int(key[0]) & 0xffffffff), np.uint64(int(key[1]) & 0xffffffff)
    for _ in range(10):
        m0, m1 = _MUL0 * c[0], _MUL1 * c[2]              # 32 x 32 -> 64 bits: no overflow in uint64
        hi0, lo0, hi1, lo1 = m0 >> _S32, m0 & _M32, m1 >> _S32, m1 & _M32
        c = [(hi1 ^ c[1] ^ a) & _M32, lo1, (hi0 ^ c[3] ^ b) & _M32, lo0]
        a, b = (a + _W0) & _M32, (b + _W1) & _M32
    return c


def words_at(seed, positions, tag):
    """uint32 draws at the given stream positions (any shape, taken modulo 2^64)."""
    pos = np.asarray(positions, dtype=np.uint64)
    flat = pos.reshape(-1)
    blk = flat >> np.uint64(2)
    seed = int(seed) & (2 ** 64 - 1)
    tag = int(tag) & (2 ** 64 - 1)
    out = philox4x32_10((blk & _M32, blk >> _S32, np.uint64(tag & 0xffffffff), np.uint64(tag >> 32)), (seed & 0xffffffff, seed >> 32))
    sel = (flat & np.uint64(3)).astype(np.int64)
    w = np.stack(out, axis=1)[np.arange(flat.size), sel]
    return w.astype(np.uint32).reshape(pos.shape)


def words(seed, first, count, tag):
    """uint32 draws first .. first + count - 1 of stream (seed, tag); `first` is a python int up to 2^64 - 1."""
    first, count = int(first) & (2 ** 64 - 1), int(count)
    if count <= 0:
        return np.zeros(0, dtype=np.uint32)
    if first + count > 2 ** 64:                                       # wraps modulo 2^64 like the device counter
        return words_at(seed, np.uint64(first) + np.arange(count, dtype=np.uint64), tag)
    # a run of positions: every block once, its four words side by side
    b0, b1 = first >> 2, (first + count - 1) >> 2
    blk = np.uint64(b0) + np.arange(b1 - b0 + 1, dtype=np.uint64)
    seed, tag = int(seed) & (2 ** 64 - 1), int(tag) & (2 ** 64 - 1)
    out = philox4x32_10((blk & _M32, blk >> _S32, np.uint64(tag & 0xffffffff), np.uint64(tag >> 32)), (seed & 0xffffffff, seed >> 32))
    flat = np.stack(out, axis=1).reshape(-1)
    lo = first - 4 * b0
    return flat[lo:lo + count].astype(np.uint32)


def u01(w):
    """The 24-bit lattice value of a word: (w >> 8) / 2^24 as fp32, in [0, 1)."""
    return ((np.asarray(w, dtype=np.uint32) >> np.uint32(8)).astype(np.float32) * np.float32(1.0 / 16777216.0)).astype(np.float32)


def uniforms(seed, first, count, tag=GATE_TAG):
    """fp32 uniforms of draws first .. first + count - 1 (the gate's stream unless another tag is named)."""
    return u01(words(seed, first, count, tag))


def _host_philox_uniforms(seed, first, count):
    """u01 of the gate's stream (counter = (block, 0x4b545550), key = seed; draw i is word i & 3 of block i >> 2; 24-bit lattice) at
    positions first .. first + count - 1."""
    return uniforms(seed, first, count, GATE_TAG)
