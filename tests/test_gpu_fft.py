"""GPU tests: hand-written Stockham FFT vs torch.fft (rocFFT oracle)."""

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def C():
    from srtb_amd.ops import native
    torch.cuda.set_device(0)
    return native()


def rand_c64(shape, seed):
    rng = np.random.default_rng(seed)
    return (rng.normal(size=shape) + 1j * rng.normal(size=shape)
            ).astype(np.complex64)


def rel_err(a, b):
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30))


# single-pass lengths
@pytest.mark.parametrize("n", [4, 64, 256, 1024, 4096])
@pytest.mark.parametrize("sign", [-1, 1])
def test_fft_single_pass(C, n, sign):
    x = rand_c64((8, n), seed=n + sign)
    xt = torch.from_numpy(x).cuda()
    out = C.native_fft(xt, sign).cpu().numpy()
    ref = (np.fft.fft(x, axis=1) if sign == -1
           else np.fft.ifft(x, axis=1) * n)
    assert rel_err(out, ref) < 2e-6 * np.sqrt(n) + 1e-5


# two-pass lengths (the waterfall backward shapes)
@pytest.mark.parametrize("n", [8192, 1 << 13, 1 << 16, 1 << 18])
@pytest.mark.parametrize("sign", [-1, 1])
def test_fft_two_pass(C, n, sign):
    batch = max(1, (1 << 20) // n)
    x = rand_c64((batch, n), seed=n % 97 + sign)
    xt = torch.from_numpy(x).cuda()
    out = C.native_fft(xt, sign).cpu().numpy()
    tt = torch.from_numpy(x).cuda()
    ref = (torch.fft.fft(tt, dim=1) if sign == -1
           else torch.fft.ifft(tt, dim=1) * n).cpu().numpy()
    assert rel_err(out, ref) < 1e-4


# multi-pass lengths (forward 2^25..2^29 class); 2^25 = balanced planner,
# 2^26/2^27/2^28 = the greedy-64 planner with remainder 0/2/4
@pytest.mark.parametrize("n", [1 << 25, 1 << 26, 1 << 27, 1 << 28])
def test_fft_three_pass(C, n):
    x = rand_c64(n, seed=5)
    xt = torch.from_numpy(x).cuda()
    out = C.native_fft(xt, -1).cpu().numpy()
    ref = torch.fft.fft(torch.from_numpy(x).cuda()).cpu().numpy()
    assert rel_err(out, ref) < 2e-4


@pytest.mark.parametrize("n", [1 << 12, 1 << 20, 1 << 24])
def test_native_rfft(C, n):
    rng = np.random.default_rng(3)
    x = rng.normal(size=n).astype(np.float32)
    xt = torch.from_numpy(x).cuda()
    out = C.native_rfft(xt).cpu().numpy()
    ref = torch.fft.rfft(xt).cpu().numpy()[:-1]
    assert rel_err(out, ref) < 1e-4


def test_native_rfft_j1644_scale(C):
    """The flagship forward shape at reduced size: 2^26 reals."""
    n = 1 << 26
    rng = np.random.default_rng(4)
    x = rng.normal(size=n).astype(np.float32)
    xt = torch.from_numpy(x).cuda()
    out = C.native_rfft(xt)
    ref = torch.fft.rfft(xt)[:-1]
    err = (out - ref).abs().max().item()
    scale = ref.abs().max().item()
    assert err < 2e-4 * scale


@pytest.mark.parametrize("maxcol", ["4", "8", "16", "64"])
def test_fft_forced_column_widths(C, maxcol, monkeypatch):
    """Every register-column width must agree with torch.fft — the balanced
    default factorization otherwise leaves N=64 (used by the 2^30 bench
    path) and small widths untested."""
    monkeypatch.setenv("SRTB_FFT_MAXCOL", maxcol)
    n = 1 << 20  # rest 14 bits over the 64 final
    x = rand_c64((2, n), seed=int(maxcol))
    xt = torch.from_numpy(x).cuda()
    out = C.native_fft(xt, -1).cpu().numpy()
    ref_t = torch.fft.fft(torch.from_numpy(x).cuda(), dim=1).cpu().numpy()
    assert rel_err(out, ref_t) < 1e-4


def test_fft_mid512_pass(C, monkeypatch):
    """The experimental 512-point strided LDS middle pass (reachable only
    through the factorization override) must match torch.fft; this exact
    plan/config was GPU-measured during round 1."""
    monkeypatch.setenv("SRTB_FFT_FACTORS", "2,512,256")
    n = 1 << 18
    x = rand_c64((4, n), seed=99)
    xt = torch.from_numpy(x).cuda()
    out = C.native_fft(xt, -1).cpu().numpy()
    ref = torch.fft.fft(torch.from_numpy(x).cuda(), dim=1).cpu().numpy()
    assert rel_err(out, ref) < 1e-4
