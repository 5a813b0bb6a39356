"""CPU checks of tests/philox_host.py, the host model every device Philox consumer is compared with: the round function against
the published Philox4x32-10 known-answer vectors (Random123's kat_vectors), and the stream layout -- word i & 3 of block i >> 2,
counter (block lo, block hi, tag lo, tag hi), key = the halves of the seed -- including positions whose block index needs more than
32 bits."""
import numpy as np

from tests import philox_host as PH

KAT = [((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
       ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
       ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1))]


def test_round_function_known_answers():
    for ctr, key, want in KAT:
        got = PH.philox4x32_10(ctr, key)
        assert tuple(int(w[0]) for w in got) == want
    # vectorised: the three vectors in one call per key
    for ctr, key, want in KAT:
        got = PH.philox4x32_10([np.array([c, c]) for c in ctr], key)
        assert all(w.tolist() == [x, x] for w, x in zip(got, want))


def test_stream_layout_and_the_carry_into_the_high_counter_word():
    seed = 0xa4093822299f31d0
    key = (seed & 0xffffffff, seed >> 32)
    for first in (0, 5, 2 ** 34 - 6, 2 ** 34, 2 ** 40 + 3, 2 ** 62, 2 ** 64 - 5):
        got = PH.words(seed, first, 11, PH.SAMPLER_TAG)
        assert got.dtype == np.uint32 and got.shape == (11,)
        for k in range(11):
            i = (first + k) % 2 ** 64
            blk = i >> 2
            blockwords = PH.philox4x32_10((blk & 0xffffffff, blk >> 32, PH.SAMPLER_TAG, 0), key)
            assert int(got[k]) == int(blockwords[i & 3][0]), (first, k)
    # a block index truncated to 32 bits would repeat the stream after 2^34 draws: it does not
    assert not np.array_equal(PH.words(seed, 2 ** 34, 8, PH.GATE_TAG), PH.words(seed, 0, 8, PH.GATE_TAG))
    assert not np.array_equal(PH.words(seed, 0, 8, PH.GATE_TAG), PH.words(seed, 0, 8, PH.SAMPLER_TAG))
    # words_at over a 2-D array of positions = words over each run
    pos = np.uint64(2 ** 34 - 3) + np.uint64(4096) * np.arange(3, dtype=np.uint64)[:, None] + np.arange(5, dtype=np.uint64)[None, :]
    at = PH.words_at(seed, pos, PH.SAMPLER_TAG)
    for b in range(3):
        assert np.array_equal(at[b], PH.words(seed, 2 ** 34 - 3 + 4096 * b, 5, PH.SAMPLER_TAG))


def test_uniforms_are_the_24_bit_lattice():
    w = PH.words(7, 2 ** 34 - 2, 1000, PH.GATE_TAG)
    u = PH.uniforms(7, 2 ** 34 - 2, 1000)
    assert u.dtype == np.float32 and float(u.min()) >= 0.0 and float(u.max()) < 1.0
    assert np.array_equal((u.astype(np.float64) * 2 ** 24).astype(np.int64), (w >> 8).astype(np.int64))
    assert np.array_equal(u, PH._host_philox_uniforms(7, 2 ** 34 - 2, 1000))
    assert np.array_equal(PH.u01(np.array([0, 255, 256, 0xffffffff], np.uint32)),
                          np.array([0.0, 0.0, 2.0 ** -24, 1.0 - 2.0 ** -24], np.float32))
