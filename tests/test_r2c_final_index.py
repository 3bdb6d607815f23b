"""Index model of the forward final pass with the r2c pair-combine at its
store (fftref.r2c_final_store, the spec of k_fft_dif_final_r2c): every
output is written exactly once, from the right two LDS elements."""

import functools

import numpy as np
import pytest

from srtb_amd import fftref

# (t, F) over the planner's factorizations of 2**t; F where P = 2**t / n
# allows 2F rows.  (13, 16) is P/2F = 1: one workgroup holds instance P/2 on
# both sides, next to the workgroup of instance 0.
CASES = [(t, f) for t in (13, 14, 16, 20) for f in (1, 8, 16, 32)
         if (1 << t) // fftref.plan_factors(t)[-1] >= 2 * f]


def test_cases_cover_the_single_workgroup_plan():
    assert (13, 16) in CASES and (13, 32) not in CASES
    assert fftref.plan_factors(13)[-1] == 256
    assert all((t, 32) in CASES for t in (14, 16, 20))


@functools.lru_cache(maxsize=None)
def packed_spectrum(t):
    """Z of a random packed input through the planner's own factorization.
    fft_deep is a Python-loop oracle (~10 M butterflies at 2**20, a minute);
    at t = 20 Z comes from numpy.fft.fft instead — what is under test is which
    elements of Z feed which output, and that holds for any Z."""
    rng = np.random.default_rng(t)
    m = 1 << t
    x = (rng.standard_normal(m) + 1j * rng.standard_normal(m)).astype(
        np.complex64)
    if t <= 16:
        return fftref.fft_deep(x, fftref.plan_factors(t), -1).astype(
            np.complex128)
    return np.fft.fft(x.astype(np.complex128))


@pytest.mark.parametrize("t,f", CASES)
def test_every_output_written_once(t, f):
    n = fftref.plan_factors(t)[-1]
    m = 1 << t
    p = m // n
    s = fftref.r2c_final_store(p, n, f)
    writes = np.bincount(s["ko"], minlength=m)
    writes += np.bincount(m - s["ko"][s["pair"] == 1], minlength=m)
    assert writes.shape == (m,)
    assert np.array_equal(writes, np.ones(m, dtype=writes.dtype))
    # the driver is the element with the smaller index
    assert s["ko"].max() == m // 2
    # both partners sit in the driver's workgroup, in the rows the kernel
    # loads there: own w*f+1+r, mirror p-(w*f+1+r), instance 0 in the last
    last = s["wg"] == p // (2 * f)
    for row, inst in ((s["row"], s["inst"]), (s["prow"], s["pinst"])):
        assert np.all(inst[last] == 0) and np.all(row[last] == 0)
        own = s["wg"] * f + 1 + row % f
        want = np.where(row < f, own, p - own)
        assert np.array_equal(inst[~last], want[~last])
        assert row.max() < 2 * f
    # the partner of output o is M - o (o = 0 pairs with itself)
    assert np.array_equal((s["pinst"] + s["pk"] * p),
                          np.where(s["ko"] == 0, 0, m - s["ko"]))
    assert np.array_equal(s["inst"] + s["k"] * p, s["ko"])


@pytest.mark.parametrize("t,f", CASES)
def test_model_spectrum_equals_r2c_post(t, f):
    n = fftref.plan_factors(t)[-1]
    z = packed_spectrum(t)
    got = fftref.r2c_final_spectrum(z, n, f)
    want = fftref.r2c_post(z, -1, dtype=np.complex128)
    assert got.dtype == want.dtype == np.complex128
    assert np.array_equal(got, want)
