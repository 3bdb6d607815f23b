"""GPU tests of the forward final pass that does the r2c pair-combine at its
store (k_fft_dif_final_r2c), against the two-kernel path it replaces
(k_fft_dif_final + k_r2c_post, SRTB_FFT_R2C_FINAL=0).

Both paths run the same butterflies and the same combine expression
(r2c_pair_combine), so the yardstick is equality bit for bit.  On top of
that, up to 2^21 the fused output meets the per-element criterion of
test_gpu_fft_accuracy.py against numpy.fft.rfft on float64:
e = max|out - ref| / rms(ref) <= 2 e_roc + 4 u, u = 2^-24, e_roc that of
torch.fft.rfft on the same input.
"""

import numpy as np
import pytest
import torch

from srtb_amd.config import Config
from srtb_amd.pipeline.cpu import synthesize_dispersed_pulse

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
SWITCH = "SRTB_FFT_R2C_FINAL"


@pytest.fixture(scope="module")
def C():
    from srtb_amd.ops import native
    torch.cuda.set_device(0)
    return native()


def inputs(n):
    """(kind, [n] float32 on the GPU).  The impulses give every bin modulus
    1, so a wrong index or twiddle shows in that bin; the constant is bin 0;
    (+1, -1, ...) is the dropped Nyquist bin, which lands in Im Z[0]."""
    g = torch.Generator(device="cuda").manual_seed(n % 1009)
    yield "noise", torch.randn(n, generator=g, device="cuda")
    for p in (1, n - 1):
        x = torch.zeros(n, device="cuda")
        x[p] = 1.0
        yield f"impulse@{p}", x
    yield "constant", torch.full((n,), 0.75, device="cuda")
    alt = torch.ones(n, device="cuda")
    alt[1::2] = -1.0
    yield "alternating", alt


def worst(out, ref):
    err = np.abs(out.astype(np.complex128) - ref).max()
    return float(err / np.sqrt((np.abs(ref) ** 2).mean()))


def bits(z):
    return torch.view_as_real(z)


# (log2 of the real length, extra environment, expected partial count or
# None).  2^14: packed 2^13 = 32 x 256, one pair workgroup holding instance
# P/2 on both sides plus the workgroup of instance 0.  2^15: final 64, two
# columns.  2^16 with 4-point columns: four prefix digits at the smallest
# size.  2^26: [64, 64, 64, 2] + 64, the flagship's plan shape.
CASES = [
    (14, {}, 2),
    (15, {}, None),
    (15, {"SRTB_FFT_DIF_F": "8"}, 256 // 16 + 1),
    (15, {"SRTB_FFT_DIF_F": "64"}, 256 // 128 + 1),
    (16, {"SRTB_FFT_MAXCOL": "4"}, None),
    (21, {}, None),
    (21, {"SRTB_FFT_DIF_F": "8"}, (1 << 14) // 16 + 1),
    (21, {"SRTB_FFT_DIF_F": "64"}, (1 << 14) // 128 + 1),
    (26, {}, None),
]


@pytest.mark.parametrize("t,env,partials", CASES,
                         ids=[f"2^{t}" + "".join(f"-{k[9:]}={v}"
                                                 for k, v in e.items())
                              for t, e, _ in CASES])
def test_fused_equals_two_kernel_path(C, monkeypatch, t, env, partials):
    n = 1 << t
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    monkeypatch.delenv(SWITCH, raising=False)
    got = C.native_rfft_final_partials(n)
    assert got > 0, "the fusion must apply here"
    if partials is not None:
        assert got == partials
    monkeypatch.setenv(SWITCH, "0")
    assert C.native_rfft_final_partials(n) == 0

    for kind, x in inputs(n):
        monkeypatch.delenv(SWITCH, raising=False)
        fused = C.native_rfft(x)
        again = C.native_rfft(x)
        monkeypatch.setenv(SWITCH, "0")
        plain = C.native_rfft(x)
        assert fused.shape == plain.shape == (n // 2,)
        diff = (bits(fused) != bits(plain)).sum().item()
        print(f"R2CFINAL len 2^{t} {env} {kind}: {diff} differing floats")
        assert torch.equal(bits(fused), bits(plain)), (kind, diff)
        # single-writer stores: a second run gives the same bits
        assert torch.equal(bits(again), bits(fused)), kind
        # (the alternating input's retained spectrum is all zeros: no scale
        # for a relative error, the bits above are its check)
        if t <= 21 and kind != "alternating":
            ref = np.fft.rfft(x.cpu().numpy().astype(np.float64))[:-1]
            e_roc = worst(torch.fft.rfft(x)[:-1].cpu().numpy(), ref)
            e = worst(fused.cpu().numpy(), ref)
            print(f"R2CFINAL len 2^{t} {kind}: e_fused {e:.3e} "
                  f"e_roc {e_roc:.3e} limit {2 * e_roc + 4 * U:.3e}")
            assert e <= 2 * e_roc + 4 * U, (kind, e, e_roc)


# ---- through the engine ----

N, S = 1 << 18, 1 << 6
ZAP = [[100, 300]]


def make_engine(C, **kw):
    args = dict(
        n=N, nbits=-8, channels=S, freq_low=1400.0, bandwidth=64.0,
        sample_rate=128e6, dm=60.0, rfi_threshold=20.0, sk_threshold=1.5,
        snr_threshold=6.0, max_boxcar=16, nsamps_reserved=0, zap_ranges=ZAP,
        use_phase_table=False, enable_rfi_s1=True, enable_sk=True, n_slots=2,
        fft_backend=0)
    args.update(kw)
    return C.PipelineEngine(**args)


@pytest.fixture(scope="module")
def pulse_and_tone():
    """A dispersed pulse at DM 60 plus a strong tone 0.3 of the way up the
    band: its bins carry ~1e4 times the mean power, far over the s1
    threshold of 20 means, so stage 1 really zaps."""
    cfg = Config()
    cfg.baseband_input_count = N
    cfg.spectrum_channel_count = S
    cfg.baseband_input_bits = -8
    cfg.baseband_freq_low = 1400.0
    cfg.baseband_bandwidth = 64.0
    cfg.baseband_sample_rate = 128e6
    cfg.dm = 60.0
    raw = synthesize_dispersed_pulse(cfg, 0.4 * N / cfg.baseband_sample_rate,
                                     pulse_amp=35.0, noise_sigma=8.0)
    tone = 20.0 * np.sin(2 * np.pi * 0.15 * np.arange(N) + 0.3)
    x = np.clip(raw.view(np.int8).astype(np.float64) + np.round(tone),
                -128, 127)
    return torch.from_numpy(x.astype(np.int8).view(np.uint8).copy())


def run_block(C, raw, **kw):
    eng = make_engine(C, **kw)
    slot = eng.submit(raw)
    res = eng.wait(slot)
    return res, eng.time_series(slot).clone(), eng.waterfall(slot).clone()


def test_engine_block_equals_two_kernel_path(C, monkeypatch, pulse_and_tone):
    raw = pulse_and_tone
    # the tone is over the stage-1 threshold in the spectrum the engine sees
    monkeypatch.setenv(SWITCH, "0")
    x = torch.from_numpy(raw.numpy().view(np.int8).astype(np.float32)).cuda()
    power = C.native_rfft(x).abs().double() ** 2
    assert (power > 20.0 * power.mean()).sum().item() >= 1

    plain = run_block(C, raw)
    monkeypatch.delenv(SWITCH, raising=False)
    assert C.native_rfft_final_partials(N) > 0
    fused = run_block(C, raw)
    assert fused[0]["counts"] == plain[0]["counts"]
    assert fused[0]["zero_count"] == plain[0]["zero_count"]
    assert torch.equal(fused[1], plain[1])
    assert torch.equal(bits(fused[2]), bits(plain[2]))


def test_engine_block_many_mean_partials(C, monkeypatch):
    """2^22 samples at one instance per side: 2^21 / 64 / 2 + 1 = 16385
    mean-power partials, more than one round of the finishing kernel's
    8 x 1024 loads (the flagship block has 131073)."""
    n = 1 << 22
    monkeypatch.setenv("SRTB_FFT_DIF_F", "1")
    rng = np.random.default_rng(22)
    x = rng.normal(0, 8, n) + 20.0 * np.sin(2 * np.pi * 0.15 * np.arange(n))
    raw = torch.from_numpy(np.clip(np.round(x), -128, 127).astype(np.int8)
                           .view(np.uint8).copy())
    monkeypatch.setenv(SWITCH, "0")
    plain = run_block(C, raw, n=n)
    monkeypatch.delenv(SWITCH, raising=False)
    assert C.native_rfft_final_partials(n) == 16385
    fused = run_block(C, raw, n=n)
    assert fused[0]["counts"] == plain[0]["counts"]
    assert fused[0]["zero_count"] == plain[0]["zero_count"]
    assert fused[0]["thresholds"] == plain[0]["thresholds"]
    assert torch.equal(fused[1], plain[1])
    assert torch.equal(bits(fused[2]), bits(plain[2]))


DMS = [0.0, 60.0, 25.0, 60.0]


def test_trials_equal_single_dm_path_with_fusion(C, monkeypatch,
                                                 pulse_and_tone):
    """test_gpu_dm_trials' expectation with the fused forward half: every
    trial equals the single-DM chain, and the repeated 60 fails if the
    spectrum the trials retain were not the ordinary one."""
    monkeypatch.delenv(SWITCH, raising=False)
    raw = pulse_and_tone
    single = make_engine(C)
    eng = make_engine(C, max_dm_trials=len(DMS))
    slot = eng.submit_trials(raw, DMS)
    got = eng.wait_trials(slot)
    plane = eng.dm_time_plane(slot)
    for k, dm in enumerate(DMS):
        s = single.submit(raw, dm_override=dm)
        want = single.wait(s)
        assert torch.equal(plane[k], single.time_series(s)), (k, dm)
        assert got[k]["counts"] == want["counts"], (k, dm)
        assert got[k]["thresholds"] == want["thresholds"], (k, dm)
        assert got[k]["zero_count"] == want["zero_count"], (k, dm)
        eng.select_trial(slot, k)
        assert torch.equal(bits(eng.waterfall(slot)),
                           bits(single.waterfall(s))), (k, dm)
