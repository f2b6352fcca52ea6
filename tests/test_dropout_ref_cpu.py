"""tests/dropout_ref.py, the host restatement of the library's dropout mask, against the constants
and formulas of csrc/rsx_common.h (hash_u32, make_dropout) and gemm_x3.hip's 32-bit keep().

tests/test_gpu_dropout_exact.py pins this restatement to the device bit for bit, for indices below
2^32. The index's HIGH word cannot be pinned to the device: that would need a tensor of more than
2^32 elements (>= 16 GiB of fp32 for one mask). Its term is covered by this file only: the general
hash equals the 32-bit shortcut when the high word is zero, and a non-zero high word changes it."""
import numpy as np
import pytest

from tests import dropout_ref as R

SEEDS = [0x123456789AD0, 4242, 777, 2 ** 61 + 12345, 5]


def _f32_below_one():
    return np.nextafter(np.float32(1.0), np.float32(0.0))


@pytest.mark.parametrize("p", [0.0, 1e-12, 0.1, 0.2, 0.5, 0.999999, float(_f32_below_one())])
def test_threshold_and_scale(p):
    """thresh = floor(double(float32(p)) * 2^32) capped at 2^32 - 1, >= 1 for p > 0, 0 for p <= 0;
    scale = 1f / (1f - float32(p)) in float32 arithmetic."""
    p32 = np.float32(p)
    t = R.threshold(p)
    s = R.scale32(p)
    assert isinstance(s, np.float32)
    if p == 0.0:
        assert t == 0 and s == np.float32(1.0)
        assert R.keep(7, p, np.arange(1000)).all()
        return
    assert 1 <= t <= 2 ** 32 - 1
    # exact integer arithmetic on float32(p) = m * 2^e
    from fractions import Fraction
    exact = Fraction(float(p32)) * 2 ** 32
    assert t == min(max(int(exact), 1), 2 ** 32 - 1)
    assert s == np.float32(1.0) / (np.float32(1.0) - p32)
    assert np.isfinite(s) and s >= 1.0


def test_threshold_known_values():
    assert R.threshold(1e-12) == 1                       # floor(2^32 * 1e-12) = 0 -> raised to 1
    assert R.threshold(0.5) == 2 ** 31
    assert R.threshold(-0.1) == 0
    assert R.threshold(0.2) == int(float(np.float32(0.2)) * 2 ** 32)   # float32(0.2), not 0.2
    assert R.threshold(0.2) != int(0.2 * 2 ** 32)
    assert R.threshold(float(_f32_below_one())) == 2 ** 32 - 2 ** 8   # (1 - 2^-24) * 2^32
    assert R.scale32(0.5) == np.float32(2.0)
    assert R.scale32(float(_f32_below_one())) == np.float32(2.0 ** 24)


def test_hash_is_fmix32_of_the_mixed_word():
    """Against an independent scalar restatement in Python integers."""
    def scalar(seed, idx):
        m = 0xFFFFFFFF
        x = (idx & m) ^ (((idx >> 32) * 0x9E3779B1) & m) ^ (seed & m)
        x ^= ((seed >> 32) * 0x85EBCA77) & m
        x ^= x >> 16
        x = (x * 0x85EBCA6B) & m
        x ^= x >> 13
        x = (x * 0xC2B2AE35) & m
        x ^= x >> 16
        return x
    rng = np.random.default_rng(0)
    idx = np.concatenate([np.arange(64, dtype=np.uint64),
                          rng.integers(0, 2 ** 63, 200, dtype=np.uint64),
                          np.array([2 ** 32 - 1, 2 ** 32, 2 ** 64 - 1], dtype=np.uint64)])
    for seed in SEEDS + [2 ** 64 - 1]:
        got = R.hash_u32(seed, idx)
        assert got.dtype == np.uint32
        assert [int(v) for v in got] == [scalar(seed, int(i)) for i in idx]
    assert R.hash_u32(0, np.array([0]))[0] == 0   # fmix32(0) = 0


@pytest.mark.parametrize("seed", SEEDS)
def test_gemm_shortcut_equals_general_hash_below_2_32(seed):
    rng = np.random.default_rng(1)
    idx = np.concatenate([np.arange(4096, dtype=np.uint64), rng.integers(0, 2 ** 32, 4096, dtype=np.uint64),
                          np.array([2 ** 32 - 1], dtype=np.uint64)])
    assert np.array_equal(R.hash_u32(seed, idx), R.hash_u32_low(seed, idx))


def test_high_words_change_the_hash():
    idx = np.arange(4096, dtype=np.uint64)
    lo = 0x9AD0
    a = R.hash_u32(lo, idx)
    b = R.hash_u32(lo | (0x1234 << 32), idx)               # seed high word
    c = R.hash_u32(lo, idx | np.uint64(1 << 32))           # index high word
    assert (a != b).mean() > 0.99 and (a != c).mean() > 0.99 and (b != c).mean() > 0.99
    # and the masks they give differ on about 2 p (1 - p) of the elements
    for other in (b, c):
        diff = ((a >= R.threshold(0.2)) != (other >= R.threshold(0.2))).mean()
        assert 0.25 < diff < 0.39, diff


@pytest.mark.parametrize("p", [0.1, 0.2, 0.5])
@pytest.mark.parametrize("n", [12288, 15232, 75776])
def test_keep_fraction_within_5_sigma(p, n):
    for seed in SEEDS:
        frac = R.keep(seed, p, np.arange(n)).mean()
        sigma = np.sqrt(p * (1 - p) / n)
        assert abs(frac - (1 - p)) <= 5 * sigma, (seed, frac, abs(frac - (1 - p)) / sigma)


def test_index_maps():
    assert R.rows_index(3, 128)[2, 5] == 2 * 128 + 5
    assert R.rows_index(3, 128, row0=10)[0, 0] == 1280
    assert R.gemm_index(131, 256)[130, 255] == 130 * 256 + 255
    ix = R.attention_index(np.array([[7, 9]]), 4, 50)
    assert ix.shape == (1, 2, 4, 50)
    assert ix[0, 1, 3, 49] == (9 * 4 + 3) * 64 + 49
    assert R.rows_keep(5, 0.2, 4, 64).shape == (4, 64)
    assert R.attention_keep(5, 0.2, np.arange(6), 2, 17).shape == (6, 2, 17)
