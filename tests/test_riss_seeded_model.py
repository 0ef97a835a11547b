"""The contract "hbmpc-riss-chacha20-v1" without a GPU: the block function it names is RFC 8439's, the model (tests/riss_seeded_model.py)
reproduces a committed fixture, its numpy form equals its scalar definition, and the range is [0, 2^lk] with the bound included."""
import json
import os

import numpy as np

from oracle.spec import _chacha20_block
from tests import riss_seeded_model as M

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "riss_seeded_v1.json")


def fixture_cases():
    """the (seed, domain, T, i, lk) of the fixture: both sides of i = 2^32, both domains with everything else equal, several sets,
    seeds and widths, and the first elements of the GPU tests' shapes that need a second block"""
    cases = []
    for seed in (M.SEED, M.sender_seed(3)):
        for domain in (0, 1):
            for T, i, lk in ((0, 0, 20), (5, 7, 20), (20, 299, 20), (0, 2**32 - 1, 1), (0, 2**32, 1), (3, 2**32 - 1, 40), (3, 2**32, 40),
                             (8191, 2**64 - 1, 59), (1, 5, 59), (2, 123456789012, 0), (2, 9, 61)):
                cases.append((seed, domain, T, i, lk))
    att = M.rows(M.SEED, 0, 21, 0, 300, 20)[1]
    for T, b in np.argwhere(att > 0)[:4]:
        cases.append((M.SEED, 0, int(T), int(b), 20))
    return cases


def test_block_function_is_rfc8439():
    """RFC 8439 section 2.3.2: key 00..1f, block counter 1, nonce 00:00:00:09 00:00:00:4a 00:00:00:00 -- state words 12..15 =
    (1, 0x09000000, 0x4a000000, 0), i.e. counter = 1 | 0x09000000 << 32 and nonce = 0x4a000000 in oracle/spec.py's arguments"""
    blk = _chacha20_block(M.seed_words(bytes(range(32))), 1 | 0x09000000 << 32, 0x4A000000)
    assert blk[0] == 0xE4E7F110 and blk[1] == 0x15593BD1 and blk[15] == 0x4E3C50A2
    # the contract's state words through the model's own call: (attempt, T | domain << 16, i mod 2^32, i div 2^32)
    T, domain, i, attempt = 0x1234, 1, (7 << 32) | 9, 2
    assert _chacha20_block(M.seed_words(M.SEED), ((T | domain << 16) << 32) + attempt, i) == \
        M._blocks(M.seed_words(M.SEED), *(np.array([w], dtype=np.uint32) for w in (attempt, 0x11234, 9, 7)))[:, 0].tolist()


def test_model_reproduces_the_fixture():
    want = json.load(open(GOLDEN))
    assert want["contract"] == "hbmpc-riss-chacha20-v1"
    cases = fixture_cases()
    assert len(want["values"]) == len(cases) >= 40
    by_key = {}
    for (seed, domain, T, i, lk), row in zip(cases, want["values"]):
        assert row[:5] == [seed.hex(), domain, T, str(i), lk]
        v, attempt = M.value_attempts(seed, domain, T, i, lk)
        assert [str(v), attempt] == row[5:], row
        assert 0 <= v <= 1 << lk
        by_key[(seed, domain, T, i, lk)] = v
    assert {2**32 - 1, 2**32} <= {c[3] for c in cases}
    # domain 0 and 1 with everything else equal differ (at a width where equal values would be a coincidence of 2^-40)
    for seed in (M.SEED, M.sender_seed(3)):
        for i in (2**32 - 1, 2**32):
            assert by_key[(seed, 0, 3, i, 40)] != by_key[(seed, 1, 3, i, 40)]
    assert any(row[6] >= 1 for row in want["values"])                         # the second block is in the fixture


def test_numpy_form_equals_the_definition():
    """rows() -- the GPU tests' reference -- against value(), element by element, across 2^32 and where attempt 1 is needed"""
    for seed, domain, Tn, first, B, lk in ((M.SEED, 0, 3, 2**32 - 3, 8, 1), (M.sender_seed(2), 1, 2, 5, 6, 59), (M.SEED, 0, 21, 0, 300, 20)):
        vals, att = M.rows(seed, domain, Tn, first, B, lk)
        assert vals.shape == att.shape == (Tn, B)
        picks = [(T, b) for T in range(Tn) for b in range(B)] if Tn * B <= 48 else \
            [(int(T), int(b)) for T, b in np.argwhere(att > 0)] + [(0, 0), (20, 299), (7, 150)]
        assert len(picks) >= 12
        for T, b in picks:
            assert (int(vals[T, b]), int(att[T, b])) == M.value_attempts(seed, domain, T, first + b, lk), (T, b)


def test_range_includes_the_bound():
    """lk = 0: values in {0, 1}; lk = 1: values in {0, 1, 2} -- the mask alone would admit 3 -- and the bound itself appears
    (prandbitd.rs:518, :766-771: the range is inclusive)"""
    for lk in (0, 1):
        vals = M.rows(M.SEED, 0, 4, 0, 300, lk)[0]
        assert int(vals.max()) == 1 << lk and int(vals.min()) == 0
        assert set(np.unique(vals).tolist()) == set(range((1 << lk) + 1))
        assert all(M.value(M.SEED, 0, T, b, lk) == int(vals[T, b]) for T, b in ((0, 0), (1, 17), (3, 299)))
