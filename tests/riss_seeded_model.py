"""The stream contract "hbmpc-riss-chacha20-v1" of the seeded RISS dealing (include/hbmpc_hip.h, csrc/kernels_riss_sample.hpp), in
Python.  value() IS the contract: the loop of the header over oracle/spec.py's ChaCha20 block function.  rows() is the same stream for
a whole [Tn][B] block in numpy (the GPU tests' reference, computed once per shape); tests/test_riss_seeded_model.py holds it to
value(), element by element."""
from functools import lru_cache

import numpy as np

from oracle.spec import _chacha20_block

SEED = bytes(range(32))  # the tests' first sender


def seed_words(seed):
    """32 bytes -> eight little-endian u32"""
    seed = bytes(seed)
    assert len(seed) == 32
    return [int.from_bytes(seed[4 * k:4 * k + 4], "little") for k in range(8)]


def sender_seed(s):
    """the tests' seed of sender s: a different one per sender; sender 0's is SEED"""
    return bytes((b + 37 * s) & 0xFF for b in range(32))


def value_attempts(seed, domain, T, i, lk):
    """(value, attempt that gave it) of (seed, domain, set index T, element index i, lk_bits)"""
    assert 0 <= T < 8192 and 0 <= domain <= 65535 and 0 <= i < 1 << 64
    key, mask, bound = seed_words(seed), (1 << (lk + 1)) - 1, 1 << lk
    attempt = 0
    while True:
        blk = _chacha20_block(key, ((T | domain << 16) << 32) + attempt, i)
        for c in range(8):
            v = (blk[2 * c] | blk[2 * c + 1] << 32) & mask
            if v <= bound:
                return v, attempt
        attempt += 1


def value(seed, domain, T, i, lk):
    return value_attempts(seed, domain, T, i, lk)[0]


def _blocks(key, w12, w13, w14, w15):
    """ChaCha20 blocks for arrays of state words 12..15 -> [16][N] uint32 (the round structure of oracle/spec.py::_chacha20_block)"""
    N = w12.shape[0]
    init = [np.full(N, c, dtype=np.uint32) for c in (0x61707865, 0x3320646E, 0x79622D32, 0x6B206574)]
    init += [np.full(N, k, dtype=np.uint32) for k in key] + [w.astype(np.uint32) for w in (w12, w13, w14, w15)]
    s = [a.copy() for a in init]

    def rotl(v, c):
        return (v << np.uint32(c)) | (v >> np.uint32(32 - c))

    def qr(a, b, c, d):
        s[a] += s[b]; s[d] = rotl(s[d] ^ s[a], 16)
        s[c] += s[d]; s[b] = rotl(s[b] ^ s[c], 12)
        s[a] += s[b]; s[d] = rotl(s[d] ^ s[a], 8)
        s[c] += s[d]; s[b] = rotl(s[b] ^ s[c], 7)

    for _ in range(10):
        qr(0, 4, 8, 12); qr(1, 5, 9, 13); qr(2, 6, 10, 14); qr(3, 7, 11, 15)
        qr(0, 5, 10, 15); qr(1, 6, 11, 12); qr(2, 7, 8, 13); qr(3, 4, 9, 14)
    return np.stack([x + y for x, y in zip(s, init)])


@lru_cache(maxsize=None)
def rows(seed, domain, Tn, first_index, B, lk):
    """(values [Tn][B] uint64, attempts [Tn][B]: the attempt that gave each value) -- one sender's hbmpc_dev_riss_sample output.
    Cached: the arrays are shared between tests and must not be written."""
    key = seed_words(seed)
    T = np.repeat(np.arange(Tn, dtype=np.uint64), B)
    i = np.tile((np.arange(B, dtype=np.uint64) + np.uint64(first_index & (2**64 - 1))), Tn)  # wraps only where the call is refused
    mask, bound = np.uint64((1 << (lk + 1)) - 1), np.uint64(1 << lk)
    out = np.zeros(Tn * B, dtype=np.uint64)
    att = np.zeros(Tn * B, dtype=np.int64)
    todo = np.arange(Tn * B)
    attempt = 0
    while todo.size:
        blk = _blocks(key, np.full(todo.size, attempt, dtype=np.uint32), (T[todo] | np.uint64(domain << 16)).astype(np.uint32),
                      (i[todo] & np.uint64(0xFFFFFFFF)).astype(np.uint32), (i[todo] >> np.uint64(32)).astype(np.uint32)).astype(np.uint64)
        found = np.zeros(todo.size, dtype=bool)
        for c in range(8):
            v = (blk[2 * c] | (blk[2 * c + 1] << np.uint64(32))) & mask
            take = ~found & (v <= bound)
            out[todo[take]], att[todo[take]] = v[take], attempt
            found |= take
        todo = todo[~found]
        attempt += 1
    out.setflags(write=False), att.setflags(write=False)
    return out.reshape(Tn, B), att.reshape(Tn, B)


def folded(seeds, domain, Tn, first_index, B, lk):
    """sums [Tn][B] over the senders' streams: hbmpc_dev_riss_sample_fold"""
    return sum(rows(bytes(s), domain, Tn, first_index, B, lk)[0] for s in seeds)
