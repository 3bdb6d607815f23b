"""The hand-written FFT per element against float64, at every power-of-two
length from 2 to 2^20, both signs, with batches that are not powers of two.

Oracle: numpy.fft on complex128 of the same float32 input.  Measure:
e = max |out - ref| / rms(ref) over the elements of a row, the largest over
the rows.  The limit is not a fixed number: torch.fft (rocFFT) transforms the
same input in the same precision with the same class of algorithm, and its
error e_roc, measured in the same test, sets the scale.  Two differently
factored float32 transforms may differ by a small factor, hence

    e_native <= 2 e_roc + 4 u,    u = 2^-24;

an index error is of order 1, and a twiddle computed in the wrong precision
grows with the length.

Inputs: unit impulses at p = (0x55555 mod len) | 1 and at p = len - 1, whose
transform exp(-+2 pi i p k / len) has unit modulus everywhere, so that every
output index and every twiddle is checked; and Gaussian noise.

Measured on an MI355X: every case is within 0.64 of its limit; the table is
in docs/fft_design.md ("Accuracy per element"), with the two twiddle
evaluations that this sweep caught below table precision.
"""

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
MAX_ELEMS = 1 << 21


@pytest.fixture(scope="module")
def C():
    from srtb_amd.ops import native
    torch.cuda.set_device(0)
    return native()


def batches(n):
    """1, 7, 37, capped so that batch * n <= 2^21.  The odd ones leave a
    tail in the wave and Stockham kernels' grids and give the column and DIF
    passes an instance count that is no multiple of their workgroup's."""
    cap = MAX_ELEMS // n
    return sorted({min(b, cap) for b in (1, 7, 37)})


def impulses(n, batch):
    x = np.zeros((batch, n), dtype=np.complex64)
    ps = [(0x55555 % n) | 1, n - 1]
    for r in range(batch):
        x[r, ps[r % 2]] = 1.0
    return x


def noise(n, batch, seed):
    rng = np.random.default_rng(seed)
    return (rng.normal(size=(batch, n)) + 1j * rng.normal(size=(batch, n))
            ).astype(np.complex64)


def inputs(n, batch, seed):
    """(kind, [batch][n]) pairs.  From 3 rows on one transform carries all
    three kinds of row; below that the kinds run one after the other."""
    if batch >= 3:
        x = noise(n, batch, seed)
        x[:2] = impulses(n, 2)
        return [("mixed", x)]
    return [("impulse", impulses(n, batch)), ("noise", noise(n, batch, seed))]


def worst(out, ref):
    """max over rows of max_k |out - ref| / rms(ref)."""
    err = np.abs(out.astype(np.complex128) - ref).max(axis=1)
    rms = np.sqrt((np.abs(ref) ** 2).mean(axis=1))
    return float((err / rms).max())


def check(C, n, sign, batch, tag=""):
    for kind, x in inputs(n, batch, seed=n % 1009 + 7 * batch + sign):
        ref = np.fft.fft(x.astype(np.complex128), axis=1)
        if sign > 0:
            ref = np.conj(np.fft.fft(np.conj(x.astype(np.complex128)), axis=1))
        xt = torch.from_numpy(x).cuda()
        roc = (torch.fft.fft(xt, dim=1) if sign < 0
               else torch.fft.ifft(xt, dim=1) * n).cpu().numpy()
        out = C.native_fft(xt, sign).cpu().numpy()
        assert out.shape == x.shape and out.dtype == np.complex64
        e_nat, e_roc = worst(out, ref), worst(roc, ref)
        print(f"FFTACC{tag} len {n} sign {sign:+d} batch {batch} {kind} "
              f"e_native {e_nat:.3e} e_roc {e_roc:.3e} "
              f"limit {2 * e_roc + 4 * U:.3e}")
        assert e_nat <= 2 * e_roc + 4 * U, (kind, e_nat, e_roc)


CASES = [(1 << t, b) for t in range(1, 21) for b in batches(1 << t)]


@pytest.mark.parametrize("sign", [-1, 1])
@pytest.mark.parametrize("n,batch", CASES)
def test_fft_per_element(C, n, batch, sign):
    check(C, n, sign, batch)


# ---- the Stockham fallbacks behind the wave and single-pass DIF kernels ----

WAVE_OFF = [(1 << t, b) for t in range(8, 13) for b in batches(1 << t)]


@pytest.mark.parametrize("sign", [-1, 1])
@pytest.mark.parametrize("n,batch", WAVE_OFF)
def test_fft_per_element_wave_off(C, n, batch, sign, monkeypatch):
    monkeypatch.setenv("SRTB_FFT_WAVE", "0")
    check(C, n, sign, batch, tag=" wave=0")


@pytest.mark.parametrize("sign", [-1, 1])
@pytest.mark.parametrize("batch", batches(4096))
def test_fft_per_element_4096_stockham(C, batch, sign, monkeypatch):
    monkeypatch.setenv("SRTB_FFT_NOSP_DIF", "1")
    check(C, 4096, sign, batch, tag=" nosp_dif=1")
