"""tests/philox_ref.py (the numpy reference the GPU tests hold the Philox kernels to) against the published known answers of
Philox4x32-10, plus the properties of the streams that the trainer relies on.  No GPU."""
import itertools

import numpy as np
import pytest

import philox_ref as PR

# Random123 kat_vectors, philox4x32 10 rounds: (counter words, key words, output words)
KAT = [
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
]


@pytest.mark.parametrize("ctr,key,out", KAT)
def test_known_answers(ctr, key, out):
    got = PR.philox4x32_10(*ctr, *key)
    assert tuple(int(w[0]) for w in got) == out


def test_known_answers_vectorised():
    """the three vectors in one call: the arithmetic is per counter, with no leak between lanes"""
    c = [np.array([k[0][j] for k in KAT], dtype=np.uint64) for j in range(4)]
    k = [np.array([k[1][j] for k in KAT], dtype=np.uint64) for j in range(2)]
    got = PR.philox4x32_10(*c, *k)
    for j in range(4):
        assert [int(v) for v in got[j]] == [kat[2][j] for kat in KAT]


def test_u01_is_the_kernels_expression():
    assert PR.u01(0xFFFFFFFF) == np.float32(1.0)                 # 16777215.5 rounds to 2^24 in float32: the range is (0, 1]
    assert PR.u01(0xFFFFFF00) == np.float32(1.0)
    assert PR.u01(0xFFFFFEFF) < np.float32(1.0)
    assert PR.u01(0) == np.float32(2.0 ** -25)
    assert PR.u01(0xFF) == np.float32(2.0 ** -25)                # the low 8 bits are dropped
    x = np.concatenate([np.arange(0, 1 << 16, dtype=np.uint64) << np.uint64(8),
                        np.arange((1 << 32) - (1 << 16), 1 << 32, 255, dtype=np.uint64)])
    u = PR.u01(x)
    assert u.dtype == np.float32 and float(u.min()) > 0.0 and float(u.max()) <= 1.0
    assert np.all(np.diff(u[:1 << 16]) > 0)                      # small arguments are exact: strictly increasing


N = 1 << 18
P = 0.3
SEED = 9 * 1000003
# the trainer's own offsets: student / teacher of iteration 0 and student of iteration 1 ((2 it + k) << 42), dropout site 1
# (site << 40), a plain small offset, and the noise offset of iteration 1 (it << 32)
OFFSETS = [0, 1 << 42, 2 << 42, 1 << 40, 77, 1 << 32]


@pytest.fixture(scope="module")
def masks():
    return {off: PR.dropout_keep(N, P, SEED, off) for off in OFFSETS}


def test_keep_rates(masks):
    for off, m in masks.items():
        rate = float(m.mean())
        print(f"offset {off:#x}: keep rate {rate:.4f}")
        assert abs(rate - (1 - P)) <= 0.005, (off, rate)


def test_streams_are_uncorrelated(masks):
    """the masks at the trainer's offsets differ in the high counter word only (or overlap shifted, for 77): a generator that
    dropped a counter word would make two of them equal (correlation 1)"""
    bound = 4.0 / np.sqrt(N)
    worst = 0.0
    for a, b in itertools.combinations(OFFSETS, 2):
        c = abs(float(np.corrcoef(masks[a].astype(np.float64), masks[b].astype(np.float64))[0, 1]))
        worst = max(worst, c)
        assert c < bound, (a, b, c, bound)
    print(f"max |corr| {worst:.4f} < {bound:.4f}")


def test_counter_is_offset_plus_index(masks):
    """offset 77 is offset 0 moved by 77 groups of four elements"""
    assert np.array_equal(masks[77][:N - 4 * 77], masks[0][4 * 77:])
    assert not np.array_equal(masks[77], masks[0])


def test_streams_and_tails():
    """the three kernels draw from different streams (c2 = 1, 2, 3); a ragged n is a prefix of the next multiple of four; the
    counter carries from c0 into c1 and the seed's high word is the second key word"""
    d = PR.dropout_keep(4096, 0.5, SEED, 0).reshape(-1, 4)[:, 0]
    c = PR.channel_keep(1024, 0.5, SEED, 0)
    assert not np.array_equal(d, c)
    assert np.array_equal(PR.dropout_keep(1001, P, SEED, 5), PR.dropout_keep(1004, P, SEED, 5)[:1001])
    a = PR.dropout_keep(16, P, SEED, (1 << 32) - 2)              # groups at counters 2^32 - 2, 2^32 - 1, 2^32, 2^32 + 1
    assert np.array_equal(a[8:], PR.dropout_keep(8, P, SEED, 1 << 32))
    w = PR.philox4x32_10(0, 1, 1, PR.C3, SEED, 0)
    assert np.array_equal(PR.dropout_keep(4, P, SEED, 1 << 32), np.array([PR.u01(x[0]) > np.float32(P) for x in w]))
    assert not np.array_equal(PR.dropout_keep(4096, P, 5, 0), PR.dropout_keep(4096, P, (1 << 40) + 5, 0))
    z = PR.noise(1 << 16, 0.1, 0.2, 42, 0)
    assert z.dtype == np.float64 and float(np.abs(z).max()) <= float(np.float32(0.2))
    assert abs(float(z.mean())) < 2e-3 and abs(float(z.std()) - 0.0954) < 2e-3      # N(0, 0.1) clamped at two sigma
    assert np.array_equal(PR.noise(1001, 0.1, 0.2, 42, 3), PR.noise(1004, 0.1, 0.2, 42, 3)[:1001])
