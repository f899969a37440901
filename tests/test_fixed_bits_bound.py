"""The fast encoder replaces libFLAC's two float bit estimates of the fixed predictor by integer forms.

libFLAC (fixed.c, FLAC__fixed_compute_best_predictor) estimates the residual bits per sample of a fixed order from
its total absolute error T over data_len = blocksize - 4 samples as

    (float)(T > 0 ? log(M_LN2 * (double)T / (double)data_len) / M_LN2 : 0.0)

and the encoder uses it twice: `bits[1] == 0.0f` gates the CONSTANT test, `bits[guess] >= subframe_bps` rules the
fixed candidate out.  k_encode_v4 codes blocks of 4096 samples only (data_len = 4092) and uses `T1 == 0` for the
first and drops the second.  Both claims are evaluated here on the expression itself, at the totals where they could
fail: the smallest totals, the integers around 4092 / ln 2 (where the logarithm crosses zero), and the largest total
4092 samples of s signed bits can reach, for every subframe sample width s of the kernel (1..17).
"""
import math

import numpy as np
import pytest

DATA_LEN = 4096 - 4
M_LN2 = np.float64(0.69314718055994530942)  # math.h
WIDTHS = range(1, 18)  # 16-bit samples less wasted bits; the side signal of a two-channel stream has 17


def fixed_bits(total):
    """libFLAC's float estimate, evaluated in double and rounded to float as the C expression is."""
    if total <= 0:
        return np.float32(0.0)
    return np.float32(np.log(M_LN2 * np.float64(total) / np.float64(DATA_LEN)) / M_LN2)


def bound(s):
    """largest total of 4092 magnitudes of samples that fit s signed bits (|x| <= 2^(s-1))"""
    return DATA_LEN * 2 ** (s - 1)


def totals():
    t = {1, 2, 5902, 5903, 5904, 5905}
    for s in WIDTHS:
        t |= {bound(s) - 1, bound(s)}
    return sorted(t)


def test_zero_crossing_is_between_integers():
    """ln 2 * T = 4092 has no integer solution: 5903 falls short of it, 5904 exceeds it, both by far more than an ulp"""
    assert M_LN2 == math.log(2.0)
    assert M_LN2 * 5903 < DATA_LEN - 0.3 and M_LN2 * 5904 > DATA_LEN + 0.3
    assert (M_LN2 * 5903) / DATA_LEN != 1.0 and (M_LN2 * 5904) / DATA_LEN != 1.0


@pytest.mark.parametrize("total", totals())
def test_estimate_is_zero_only_for_zero_total(total):
    fb = fixed_bits(total)
    print(f"T = {total}: estimate {fb!r}")
    assert fb != np.float32(0.0)
    assert abs(float(fb)) >= 1e-4  # nowhere near a float that could round or flush to zero
    assert fixed_bits(0) == np.float32(0.0)


@pytest.mark.parametrize("s", WIDTHS)
def test_estimate_stays_below_sample_width(s):
    for total in totals():
        if total > bound(s):
            continue
        fb = fixed_bits(total)
        print(f"s = {s}, T = {total}: estimate {fb!r}")
        assert not (fb >= np.float32(s))
        assert float(fb) < s - 1.5  # log2(T ln 2 / 4092) <= s - 1 + log2(ln 2) = s - 1.53
