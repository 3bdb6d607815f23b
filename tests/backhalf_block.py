"""The crafted block of the back-half tests (test_gpu_backhalf.py,
test_backhalf_fixture.py) and its float64 oracle.

One int8 block of N = 2^18 samples at 128 Msps that makes every stage of the
engine's back half do something:

  noise        Gaussian, sigma 8
  pulse        a band-filling click at DM 10: detections at every boxcar length
  chirp        constant envelope, sweeps across 0.1 .. 0.9 of waterfall row 2
               during the block: its row's spectral kurtosis falls below the
               lower threshold; spread over many bins, it stays far below the
               RFI-s1 threshold
  gated tone   at the centre frequency of row S - 3, on for N / 256 samples:
               that row's spectral kurtosis rises above the upper threshold
  CW           exactly on one spectrum bin: zapped by RFI s1

Waterfall row r holds the baseband frequencies r / (2 S) .. (r + 1) / (2 S)
cycles per sample.
"""

import numpy as np

from srtb_amd import ref
from srtb_amd.config import Config
from srtb_amd.pipeline.cpu import synthesize_dispersed_pulse

N = 1 << 18
FREQ_LOW, BANDWIDTH, SAMPLE_RATE = 1400.0, 64.0, 128e6
DM = 10.0
RFI_THRESHOLD = 20.0
SK_THRESHOLD = 1.5
SNR_THRESHOLD = 6.0
MAX_BOXCAR = 16
ZAP = [[100, 300]]  # inclusive spectrum bins
CHIRP_ROW = 2
CW_BIN = int(0.41 * N / 2)


def tone_row(S):
    return S - 3


def reserved(S):
    """nsamps_reserved = 3 S drops 3 waterfall columns: ts_count is odd."""
    return 3 * S


def block_config(S):
    cfg = Config()
    cfg.baseband_input_count = N
    cfg.spectrum_channel_count = S
    cfg.baseband_input_bits = -8
    cfg.baseband_freq_low = FREQ_LOW
    cfg.baseband_bandwidth = BANDWIDTH
    cfg.baseband_sample_rate = SAMPLE_RATE
    cfg.dm = DM
    return cfg


def make_block(S):
    """uint8 view of the int8 block, NumPy [N]."""
    raw = synthesize_dispersed_pulse(
        block_config(S), 0.3 * N / SAMPLE_RATE, pulse_amp=0.4, noise_sigma=8.0,
        rng=np.random.default_rng(0), width=1)
    t = np.arange(N, dtype=np.float64)
    f0, f1 = (CHIRP_ROW + 0.1) / (2 * S), (CHIRP_ROW + 0.9) / (2 * S)
    chirp = 8.0 * np.sqrt(10.0 / S) * np.cos(
        2 * np.pi * (f0 * t + 0.5 * (f1 - f0) * t * t / N))
    gate = (t >= int(0.6 * N)) & (t < int(0.6 * N) + N // 256)
    tone = 24.0 * np.cos(2 * np.pi * (tone_row(S) + 0.5) / (2 * S) * t) * gate
    cw = 3.0 * np.cos(2 * np.pi * CW_BIN / N * t)
    x = raw.view(np.int8).astype(np.float64) + np.round(chirp + tone + cw)
    return np.clip(x, -128, 127).astype(np.int8).view(np.uint8).copy()


WINDOWED_SK_THRESHOLD = 4.0  # see test_windowed_block_margins


def make_noise_block():
    """Gaussian noise only, sigma 8 (the windowed case)."""
    rng = np.random.default_rng(0)
    return np.clip(np.round(rng.normal(0, 8.0, N)), -128, 127).astype(
        np.int8).view(np.uint8).copy()


def sk_thresholds(L, sk_threshold=SK_THRESHOLD):
    """(lo', hi') of ref.rfi_mitigate_sk, rounded to float32 as the engine
    rounds them."""
    hi = float(sk_threshold)
    lo = 2.0 - hi
    if lo > hi:
        lo, hi = hi, lo
    corr = (L - 1.0) / (L + 1.0)
    return float(np.float32(lo * corr + 1.0)), float(np.float32(hi * corr + 1.0))


def boxcar_lengths(ts_count, max_boxcar=MAX_BOXCAR):
    out, b = [], 2
    while b <= max_boxcar and b < ts_count:
        out.append(b)
        b *= 2
    return out


def oracle(raw, S, window=None, sk_threshold=SK_THRESHOLD):
    """The whole chain in float64 / complex128.  window: None or "hamming"
    (applied to the samples, de-applied on the waterfall rows)."""
    x = raw.view(np.int8).astype(np.float64)
    if window:
        x = x * ref.window_coefficients(window, N, np.float64)
    nc = N // 2
    L = nc // S
    spec = np.fft.rfft(x)[:-1]
    power = spec.real ** 2 + spec.imag ** 2
    mean = power.mean()
    ratio = power / mean
    spec = np.where(ratio > RFI_THRESHOLD, 0.0, spec * (nc * nc / S) ** -0.5)
    for lo, hi in ZAP:
        spec[lo:hi + 1] = 0
    f = FREQ_LOW + BANDWIDTH / nc * np.arange(nc, dtype=np.float64)
    f_c = FREQ_LOW + BANDWIDTH
    k = ref.D_DISPERSION * 1e6 * DM / f * ((f - f_c) / f_c) ** 2
    spec = spec * np.exp(-2j * np.pi * (k - np.trunc(k)))
    wf = np.fft.ifft(spec.reshape(S, L), axis=1) * L
    if window:
        wf = wf / ref.window_coefficients(window, L, np.float64)[None, :]
    p = wf.real ** 2 + wf.imag ** 2
    s2, s4 = p.sum(axis=1), (p * p).sum(axis=1)
    sk = L * s4 / (s2 * s2)
    lo_, hi_ = sk_thresholds(L, sk_threshold)
    flags = (sk > hi_) | (sk < lo_) | (s2 == 0)
    ts_count = L - reserved(S) // S
    ts = p[~flags, :ts_count].sum(axis=0)
    ts = ts - ts.mean()
    cum = np.cumsum(ts)
    counts = {1: int((ts > SNR_THRESHOLD * np.sqrt((ts * ts).mean())).sum())}
    for b in boxcar_lengths(ts_count):
        box = cum[b:] - cum[:-b]
        counts[b] = int((box > SNR_THRESHOLD * np.sqrt((box * box).mean())).sum())
    return {"rfi_ratio": ratio, "sk": sk, "sk_lo": lo_, "sk_hi": hi_,
            "flags": flags, "time_series": ts, "counts": counts}
