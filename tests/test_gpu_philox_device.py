"""The device's Philox4x32-10 in the form the sphere-only render builds run it (philox_ukeys: the wave-uniform key is
re-added per call instead of held as eighteen round keys in SGPRs) must give the oracle's words, word
for word: the Random123 known-answer vectors of tests/test_oracle_kat.py and 65 536 seeded random (counter, key) pairs,
among the keys 0, 0xFFFFFFFF and values whose key schedule wraps 2^32 in both halves."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

W0, W1 = 0x9E3779B9, 0xBB67AE85           # the key schedule's increments (Weyl constants)

KAT = [([0, 0, 0, 0], [0, 0], [0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8]),
       ([0xFFFFFFFF] * 4, [0xFFFFFFFF] * 2, [0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD]),
       ([0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344], [0xA4093822, 0x299F31D0], [0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1])]


def _oracle_words(oracle, counters, keys):
    fn = oracle.lib().bto_philox4x32_10
    out = np.zeros((counters.shape[0], 4), np.uint32)
    c, k, o = (C.c_uint32 * 4)(), (C.c_uint32 * 2)(), (C.c_uint32 * 4)()
    for i in range(counters.shape[0]):
        c[:] = counters[i].tolist()
        k[:] = keys[i].tolist()
        fn(c, k, o)
        out[i] = o[:]
    return out


def test_known_answer_vectors(bendy):
    got = bendy.Tracer.philox_device([c for c, _, _ in KAT], [k for _, k, _ in KAT])
    assert got.tolist() == [w for _, _, w in KAT]


def test_random_pairs_equal_the_oracle(bendy, oracle):
    rng = np.random.default_rng(0x5EED)
    n = 65536
    counters = rng.integers(0, 1 << 32, (n, 4), dtype=np.uint64).astype(np.uint32)
    keys = rng.integers(0, 1 << 32, (n, 2), dtype=np.uint64).astype(np.uint32)
    # keys at the edges: 0, all ones, and for every round i = 1 .. 9 the keys whose schedule passes 2^32 exactly there
    # (k + i * W = 2^32 - 1, 2^32 and 2^32 + 1 (mod 2^32)), in both halves at once and in one half only
    special = [(0, 0), (0xFFFFFFFF, 0xFFFFFFFF), (0, 0xFFFFFFFF), (0xFFFFFFFF, 0)]
    for i in range(1, 10):
        for d in (-1, 0, 1):
            k0, k1 = (d - i * W0) % (1 << 32), (d - i * W1) % (1 << 32)
            special += [(k0, k1), (k0, 0x12345678), (0x9ABCDEF0, k1)]
    keys[:len(special)] = np.asarray(special, np.uint64).astype(np.uint32)
    counters[:4] = [[0, 0, 0, 0], [0xFFFFFFFF] * 4, [0, 0xFFFFFFFF, 0, 0xFFFFFFFF], [0xFFFFFFFF, 0, 0xFFFFFFFF, 0]]
    want = _oracle_words(oracle, counters, keys)
    got = bendy.Tracer.philox_device(counters, keys)
    bad = np.flatnonzero((got != want).any(axis=1))
    assert bad.size == 0, (bad[:8].tolist(), got[bad[:2]].tolist(), want[bad[:2]].tolist())


def test_a_count_that_is_no_multiple_of_the_wave(bendy, oracle):
    rng = np.random.default_rng(7)
    n = 64 * 5 + 37                        # a ragged last wave, more than one block
    counters = rng.integers(0, 1 << 32, (n, 4), dtype=np.uint64).astype(np.uint32)
    keys = rng.integers(0, 1 << 32, (n, 2), dtype=np.uint64).astype(np.uint32)
    assert np.array_equal(bendy.Tracer.philox_device(counters, keys), _oracle_words(oracle, counters, keys))
