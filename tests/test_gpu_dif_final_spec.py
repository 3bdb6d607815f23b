"""GPU tests of the length-64 final passes with compile-time n and F
(k_fft_dif64_final, k_fft_dif64_final_r2c) against the generic kernels they
stand in for (k_fft_dif_final, k_fft_dif_final_r2c; SRTB_FFT_DIF_SPEC=0).

The specialised kernels run the generic kernels' arithmetic in the generic
kernels' order, so every comparison is bit for bit: outputs, SK sums, and
through the engine the mean power that sets the stage-1 threshold.  Values
of F that have no specialised instance (8, 64) must take the generic kernel
without notice.

One case asked for cannot be built: a batch with n_ffts % 32 != 0.  A plan
that ends in a length-64 final pass has length >= 2^13, so every batch row
holds a multiple of 128 instances and F = 32 is never clamped; the smallest
such plan (2^13 with SRTB_FFT_FINAL=64, 128 instances per row) and odd
batches stand in for it.
"""

import pytest
import torch

from tests.test_gpu_r2c_final import (bits, inputs, make_engine,  # noqa: F401
                                      pulse_and_tone, run_block)

pytestmark = pytest.mark.gpu

SPEC = "SRTB_FFT_DIF_SPEC"


@pytest.fixture(scope="module")
def C():
    from srtb_amd.ops import native
    torch.cuda.set_device(0)
    return native()


def both(monkeypatch, fn):
    """fn() under the generic kernels, then under the specialised ones."""
    monkeypatch.setenv(SPEC, "0")
    generic = fn()
    monkeypatch.delenv(SPEC, raising=False)
    return generic, fn()


def c2c_inputs(batch, n):
    g = torch.Generator(device="cuda").manual_seed(batch * 131 + n % 1009)
    yield "noise", torch.view_as_complex(
        torch.randn(batch, n, 2, generator=g, device="cuda"))
    for p in (1, n - 1):
        x = torch.zeros(batch, n, dtype=torch.complex64, device="cuda")
        x[:, p] = 1.0 - 0.5j
        yield f"impulse@{p}", x
    yield "constant", torch.full((batch, n), 0.75 + 0.25j,
                                 dtype=torch.complex64, device="cuda")


# (log2 length, plan environment).  2^13 with a length-64 final: 128
# instances per row, the fewest a length-64 final pass can meet.  2^14:
# the smallest default plan ending in one.  2^18: the waterfall's plan.
# 2^16 with 4-point columns: four prefix digits.
C2C_PLANS = [
    (13, {"SRTB_FFT_FINAL": "64"}),
    (14, {}),
    (15, {}),
    (18, {}),
    (16, {"SRTB_FFT_MAXCOL": "4"}),
]
F_VALUES = [None, "8", "16", "32", "64"]


@pytest.mark.parametrize("f", F_VALUES, ids=lambda f: f"F={f}")
@pytest.mark.parametrize("t,env", C2C_PLANS,
                         ids=[f"2^{t}" + "".join(f"-{k[9:]}={v}"
                                                 for k, v in e.items())
                              for t, e in C2C_PLANS])
def test_c2c_equals_generic(C, monkeypatch, t, env, f):
    n = 1 << t
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    if f is not None:
        monkeypatch.setenv("SRTB_FFT_DIF_F", f)
    for batch in (1, 3, 7):
        for kind, x in c2c_inputs(batch, n):
            for sign in (-1, 1):
                generic, spec = both(monkeypatch,
                                     lambda: C.native_fft(x, sign))
                diff = (bits(spec) != bits(generic)).sum().item()
                if diff:
                    print(f"DIF64 c2c 2^{t} {env} F={f} batch {batch} "
                          f"{kind} sign {sign}: {diff} differing floats")
                assert diff == 0, (batch, kind, sign, diff)
                if kind == "noise":
                    # the transform is the right one, not merely the same
                    # one: float32 error is O(2^-24 log2 n) of the rms, far
                    # inside 1e-5 of the largest bin
                    xd = x.to(torch.complex128)
                    ref = (torch.fft.fft(xd) if sign < 0
                           else torch.fft.ifft(xd) * n)
                    err = (spec.to(torch.complex128) - ref).abs().max()
                    assert err <= 1e-5 * ref.abs().max(), (batch, sign, err)


@pytest.mark.parametrize("rows,t", [(64, 14), (8, 15)])
def test_sk_sums_equal_generic(C, monkeypatch, rows, t):
    n = 1 << t
    g = torch.Generator(device="cuda").manual_seed(rows + t)
    x = torch.view_as_complex(
        torch.randn(rows, n, 2, generator=g, device="cuda"))
    x[1] *= 3.0  # rows with different sums
    generic, spec = both(monkeypatch, lambda: C.native_fft_sk(x))
    assert torch.equal(bits(spec[0]), bits(generic[0]))
    assert spec[1].shape == (rows, 2)
    diff = (spec[1] != generic[1]).sum().item()
    print(f"DIF64 sk {rows} x 2^{t}: {diff} differing sums")
    assert torch.equal(spec[1], generic[1])
    assert (generic[1][:, 0] > 0).all()


# (log2 real length, plan environment).  2^14 packs to 32 x 256: the generic
# kernel on both sides, which must still pass.
R2C_PLANS = [
    (14, {}),
    (15, {}),
    (16, {"SRTB_FFT_MAXCOL": "4"}),
    (21, {}),
]


@pytest.mark.parametrize("f", [None, "16", "32"], ids=lambda f: f"F={f}")
@pytest.mark.parametrize("t,env", R2C_PLANS,
                         ids=[f"2^{t}" + "".join(f"-{k[9:]}={v}"
                                                 for k, v in e.items())
                              for t, e in R2C_PLANS])
def test_r2c_equals_generic(C, monkeypatch, t, env, f):
    n = 1 << t
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    if f is not None:
        monkeypatch.setenv("SRTB_FFT_R2C_F", f)
    assert C.native_rfft_final_partials(n) > 0
    for kind, x in inputs(n):
        generic, spec = both(monkeypatch, lambda: C.native_rfft(x))
        again = C.native_rfft(x)
        for name, got in (("spec", spec), ("again", again)):
            diff = (bits(got) != bits(generic)).sum().item()
            if diff:
                print(f"DIF64 r2c 2^{t} {env} F={f} {kind} {name}: "
                      f"{diff} differing floats")
            assert diff == 0, (kind, name, diff)


@pytest.mark.parametrize("dm", [60.0, -60.0])
def test_engine_block_equals_generic(C, monkeypatch, pulse_and_tone, dm):
    """N = 2^18, S = 2^6, SK on: the forward final pass writes the mean
    partials that set the stage-1 threshold (the waterfall rows of 2^11 are
    single-pass; test_sk_sums_equal_generic has the SK instance)."""
    raw = pulse_and_tone
    generic, spec = both(monkeypatch, lambda: run_block(C, raw, dm=dm))
    assert spec[0]["counts"] == generic[0]["counts"]
    assert spec[0]["zero_count"] == generic[0]["zero_count"]
    assert spec[0]["thresholds"] == generic[0]["thresholds"]
    assert torch.equal(spec[1], generic[1])
    assert torch.equal(bits(spec[2]), bits(generic[2]))
