"""NumPy reference implementations of every device operation.

These are the *oracles*: each HIP/CDNA4 kernel in ``csrc/kernels`` is tested
against the function of the same name here, and the CPU pipeline path
(:mod:`srtb_amd.pipeline.cpu`) is built from them.  Semantics mirror the
reference implementation (file:line cited per function) so that detection
thresholds and output products transfer; the GPU code is an independent
MI355X-native design that must only agree numerically.

All functions are pure; complex spectra are complex64 unless stated otherwise.
FFT conventions follow cuFFT/hipFFT (forward unscaled, backward unscaled) —
NumPy's ``ifft`` is multiplied back by ``n``.
"""

from __future__ import annotations

import math

import numpy as np

# Dispersion constant, MHz^2 pc^-1 cm^3 s
# (reference: userspace/include/srtb/coherent_dedispersion.hpp:67 — the
# "accurate" value 4.148808e3, not tempo2's 4.149378e3)
D_DISPERSION = 4.148808e3

# ---------------------------------------------------------------------------
# FFT windows (reference: userspace/include/srtb/fft/fft_window.hpp:27-110)
# ---------------------------------------------------------------------------


def window_coefficients(kind: str, n: int, dtype=np.float32) -> np.ndarray:
    """Window coefficient table: coef[i] = w(i / (n-1)), i in [0, n).

    kind: "rectangle" (default in the reference), "hann", "hamming".
    cosine-sum form: w(x) = sum_k (-1)^k a_k cos(2 pi k x).
    """
    x = np.arange(n, dtype=np.float64) / max(n - 1, 1)
    if kind == "rectangle":
        w = np.ones(n, dtype=np.float64)
    elif kind == "hann":
        w = 0.5 - 0.5 * np.cos(2 * np.pi * x)
    elif kind == "hamming":
        w = 25.0 / 46.0 - 21.0 / 46.0 * np.cos(2 * np.pi * x)
    else:
        raise ValueError(f"unknown window {kind!r}")
    return w.astype(dtype)


# ---------------------------------------------------------------------------
# Unpack (reference: userspace/include/srtb/unpack.hpp:43-403)
# ---------------------------------------------------------------------------


def unpack(data: np.ndarray, nbits: int, window: np.ndarray | None = None,
           dtype=np.float32) -> np.ndarray:
    """Unpack packed baseband bytes to float samples.

    ``nbits``: 1, 2, 4 → unsigned sub-byte fields, MSB-first within each byte
    (reference unpack.hpp:43-140); 8 → uint8 cast; -8 → int8 cast; 16/-16,
    32/-32 → u/int casts (unpack.hpp:143-156).  ``window`` (optional) is
    multiplied element-wise (the reference fuses the FFT window here).
    """
    data = np.asarray(data)
    if nbits in (1, 2, 4):
        b = np.frombuffer(data.tobytes(), dtype=np.uint8)
        per = 8 // nbits
        shifts = np.arange(per - 1, -1, -1, dtype=np.uint8) * nbits
        mask = (1 << nbits) - 1
        out = ((b[:, None] >> shifts[None, :]) & mask).reshape(-1).astype(dtype)
    elif abs(nbits) == 8:
        b = np.frombuffer(data.tobytes(), dtype=np.int8 if nbits < 0 else np.uint8)
        out = b.astype(dtype)
    elif abs(nbits) == 16:
        b = np.frombuffer(data.tobytes(), dtype=np.int16 if nbits < 0 else np.uint16)
        out = b.astype(dtype)
    elif abs(nbits) == 32:
        b = np.frombuffer(data.tobytes(), dtype=np.int32 if nbits < 0 else np.uint32)
        out = b.astype(dtype)
    else:
        raise ValueError(f"unsupported nbits {nbits}")
    if window is not None:
        out = (out * window[: out.size]).astype(dtype)
    return out


def unpack_interleaved_2pol(data: np.ndarray, window: np.ndarray | None = None,
                            dtype=np.float32) -> tuple[np.ndarray, np.ndarray]:
    """int8 samples interleaved sample-by-sample: p0 s0, p1 s0, p0 s1, ...

    (reference unpack.hpp:221-244).  Returns (pol0, pol1)."""
    b = np.frombuffer(np.asarray(data).tobytes(), dtype=np.int8).astype(dtype)
    p0, p1 = b[0::2].copy(), b[1::2].copy()
    if window is not None:
        p0 = (p0 * window[: p0.size]).astype(dtype)
        p1 = (p1 * window[: p1.size]).astype(dtype)
    return p0, p1


def unpack_naocpsr_snap1(data: np.ndarray, window: np.ndarray | None = None,
                         dtype=np.float32) -> tuple[np.ndarray, np.ndarray]:
    """SNAP-1 "1 1 2 2" interleave: 2 int8 samples per pol alternating
    (reference unpack.hpp:255-283).  Returns (pol0, pol1)."""
    b = np.frombuffer(np.asarray(data).tobytes(), dtype=np.int8)
    b = b.reshape(-1, 4)  # [s0p0, s1p0, s0p1, s1p1]
    p0 = b[:, 0:2].reshape(-1).astype(dtype)
    p1 = b[:, 2:4].reshape(-1).astype(dtype)
    if window is not None:
        p0 = (p0 * window[: p0.size]).astype(dtype)
        p1 = (p1 * window[: p1.size]).astype(dtype)
    return p0, p1


def unpack_gznupsr_a1(data: np.ndarray, n_streams: int = 2,
                      window: np.ndarray | None = None,
                      dtype=np.float32) -> list[np.ndarray]:
    """GZNU ZCU111 4-byte-word deinterleave (reference unpack.hpp:291-403).

    Packet payload is a sequence of 4-byte words cycling over ``n_streams``
    ADCs; each word holds 4 consecutive samples of one stream.  The 4-stream
    (v1) variant stores offset-binary bytes, fixed by XOR 0x80; the 2-stream
    (v2, current) variant is plain int8.
    """
    b = np.frombuffer(np.asarray(data).tobytes(), dtype=np.uint8)
    words = b.reshape(-1, n_streams, 4)
    outs = []
    for s in range(n_streams):
        v = words[:, s, :].reshape(-1)
        if n_streams == 4:
            v = v ^ np.uint8(0x80)
        v = v.astype(np.int8).astype(dtype)
        if window is not None:
            v = (v * window[: v.size]).astype(dtype)
        outs.append(v)
    return outs


# ---------------------------------------------------------------------------
# FFT stages (library in the GPU path; NumPy here, cuFFT scaling convention)
# ---------------------------------------------------------------------------


def fft_r2c_drop_nyquist(x: np.ndarray) -> np.ndarray:
    """Forward R2C of the full block, dropping the Nyquist bin so the output
    count is exactly N/2 (reference fft_pipe.hpp:77 'drop the highest
    frequency point')."""
    X = np.fft.rfft(np.asarray(x, dtype=np.float64))
    return X[:-1].astype(np.complex64)


def waterfall_ifft(spec: np.ndarray, n_channels: int) -> np.ndarray:
    """Batched backward C2C over contiguous chunks: the Nc-bin dedispersed
    spectrum is viewed as [n_channels][L] (L = Nc / n_channels contiguous fine
    bins per coarse channel) and each row is inverse-FFT'd to L time samples
    (reference watfft_1d_c2c_pipe, fft_pipe.hpp:294-311).  cuFFT backward is
    unscaled, hence the * L."""
    spec = np.asarray(spec)
    nc = spec.size
    L = nc // n_channels
    m = spec.reshape(n_channels, L)
    out = np.fft.ifft(m, axis=1) * L
    return out.astype(np.complex64)


# ---------------------------------------------------------------------------
# RFI mitigation stage 1 (reference: pipeline/rfi_mitigation_pipe.hpp:50-101,
# spectrum/rfi_mitigation.hpp:42-157)
# ---------------------------------------------------------------------------


def rfi_mitigate_s1(spec: np.ndarray, threshold: float,
                    spectrum_channel_count: int) -> np.ndarray:
    """Zap bins with |X|^2 > threshold * mean(|X|^2); scale survivors by
    (Nc^2 / S)^(-1/2) (normalization fused in, rfi_mitigation_pipe.hpp:60-80)."""
    spec = np.asarray(spec)
    n = spec.size
    power = (spec.real.astype(np.float64)) ** 2 + (spec.imag.astype(np.float64)) ** 2
    avg = power.mean()
    coeff = (float(n) * float(n) / float(spectrum_channel_count)) ** -0.5
    out = np.where(power > threshold * avg, 0.0, spec * coeff)
    return out.astype(spec.dtype)


def rfi_ranges_to_bins(freq_low: float, bandwidth: float, n_bins: int,
                       ranges: list[tuple[float, float]]) -> list[tuple[int, int]]:
    """Map RFI frequency ranges (MHz) to inclusive bin index ranges
    (reference spectrum/rfi_mitigation.hpp:97-157; bin i sits at
    freq_low + bandwidth * i / (n_bins - 1); handles negative bandwidth)."""
    out = []
    bw_neg = bandwidth < 0
    for lo, hi in ranges:
        if (hi - lo < 0) != bw_neg:
            lo, hi = hi, lo
        i_lo = int(round((lo - freq_low) / bandwidth * (n_bins - 1)))
        i_hi = int(round((hi - freq_low) / bandwidth * (n_bins - 1)))
        if 0 <= i_lo <= i_hi < n_bins:
            out.append((i_lo, i_hi))
        # else: out of band -> warn and skip (reference logs a warning)
    return out


def parse_rfi_freq_list(text: str) -> list[tuple[float, float]]:
    """Parse "11-12, 15-90" style lists (reference eval_rfi_ranges)."""
    ranges = []
    for part in text.split(","):
        part = part.strip()
        if not part:
            continue
        nums = [p for p in part.split("-") if p != ""]
        if len(nums) != 2:
            continue  # reference logs a warning and skips
        ranges.append((float(nums[0]), float(nums[1])))
    return ranges


def rfi_mitigate_manual(spec: np.ndarray, freq_low: float, bandwidth: float,
                        ranges: list[tuple[float, float]]) -> np.ndarray:
    spec = np.asarray(spec).copy()
    for i_lo, i_hi in rfi_ranges_to_bins(freq_low, bandwidth, spec.size, ranges):
        spec[i_lo : i_hi + 1] = 0
    return spec


# ---------------------------------------------------------------------------
# Coherent dedispersion (reference: coherent_dedispersion.hpp:40-248)
# ---------------------------------------------------------------------------


def dedisp_phase_factors(n: int, f_min: float, f_c: float, df: float,
                         dm: float) -> np.ndarray:
    """Phase factor per frequency bin, computed in float64 like the reference's
    phase_factor_v3: k = D*1e6 * dm / f * ((f-f_c)/f_c)^2 (cycles; may be ~1e9),
    factor = exp(-2*pi*i*frac(k)).  f = f_min + df*i, frequencies in MHz."""
    i = np.arange(n, dtype=np.float64)
    f = f_min + df * i
    delta_f = f - f_c
    k = (D_DISPERSION * 1e6) * dm / f * (delta_f / f_c) ** 2
    k_frac = k - np.trunc(k)  # C modf keeps the sign, like trunc
    delta_phi = -2.0 * np.pi * k_frac
    return (np.cos(delta_phi) + 1j * np.sin(delta_phi)).astype(np.complex64)


def coherent_dedisperse(spec: np.ndarray, f_min: float, f_c: float, df: float,
                        dm: float) -> np.ndarray:
    spec = np.asarray(spec)
    factors = dedisp_phase_factors(spec.size, f_min, f_c, df, dm)
    return (spec * factors).astype(spec.dtype)


def dispersion_delay_time(f: float, f_c: float, dm: float) -> float:
    """Delay (s) of frequency f relative to f_c (MHz), positive when f > f_c
    (reference coherent_dedispersion.hpp:76-79)."""
    return -D_DISPERSION * dm * (1.0 / (f * f) - 1.0 / (f_c * f_c))


def nsamps_reserved(baseband_input_count: int, spectrum_channel_count: int,
                    freq_low: float, bandwidth: float, sample_rate: float,
                    dm: float, reserve: bool = True,
                    time_multiple: int = 1) -> int:
    """Overlap (in real samples) between adjacent blocks so dedispersion edge
    garbage can be dropped; the valid region is rounded down to a multiple of
    2 * spectrum_channel_count (reference coherent_dedispersion.hpp:87-128).
    ``time_multiple`` = t rounds it down to a multiple of
    2 * spectrum_channel_count * t instead, so that the valid waterfall
    columns of a block divide into whole groups of t (filterbank tscrunch)."""
    if not reserve:
        return 0
    max_delay = dispersion_delay_time(freq_low + bandwidth, freq_low, dm)
    minimal = 2 * round(max_delay * sample_rate)
    per_bin = 2 * spectrum_channel_count * time_multiple
    refft_total = (baseband_input_count - minimal) // per_bin * per_bin
    n_may = baseband_input_count - refft_total
    if refft_total > 0:
        return int(n_may)
    return 0  # reference warns and disables overlap


# ---------------------------------------------------------------------------
# Spectral kurtosis RFI (stage 2)
# (reference: spectrum/rfi_mitigation.hpp:183-340)
# ---------------------------------------------------------------------------


def spectral_kurtosis_sk(wf: np.ndarray) -> np.ndarray:
    """SK statistic per frequency row of a [n_channels][M] waterfall:
    SK = M * S4 / S2^2 with S2 = sum |x|^2, S4 = sum |x|^4."""
    wf = np.asarray(wf)
    p = (wf.real.astype(np.float64)) ** 2 + (wf.imag.astype(np.float64)) ** 2
    s2 = p.sum(axis=1)
    s4 = (p * p).sum(axis=1)
    M = wf.shape[1]
    with np.errstate(divide="ignore", invalid="ignore"):
        sk = M * s4 / (s2 * s2)
    return sk


def sk_flags(wf: np.ndarray, sk_threshold: float) -> np.ndarray:
    """Boolean [n_channels]: rows whose SK is outside the corrected
    [lo', hi'] band; lo = 2 - thr, hi = thr, x' = x*(M-1)/(M+1) + 1
    (reference rfi_mitigation.hpp:292-340)."""
    wf = np.asarray(wf)
    M = wf.shape[1]
    hi = float(sk_threshold)
    lo = 2.0 - hi
    if lo > hi:
        lo, hi = hi, lo
    corr = (M - 1.0) / (M + 1.0)
    lo_, hi_ = lo * corr + 1.0, hi * corr + 1.0
    sk = spectral_kurtosis_sk(wf)
    return (sk > hi_) | (sk < lo_)


def rfi_mitigate_sk(wf: np.ndarray, sk_threshold: float) -> np.ndarray:
    """Method 2: zero whole frequency rows that sk_flags() marks."""
    wf = np.asarray(wf).copy()
    wf[sk_flags(wf, sk_threshold), :] = 0
    return wf


def rfi_mitigate_sk_v1(wf_tf: np.ndarray, sk_threshold: float,
                       normalize: bool = False) -> np.ndarray:
    """Method 1 (reference rfi_mitigation.hpp:183-274): TIME-MAJOR layout
    [M][fft_bins] (one thread per frequency bin walks the M time samples of
    its column), same corrected SK thresholds as method 2, zeroing whole
    frequency columns; optional per-column normalization by sqrt(mean |x|^2)
    of the surviving data."""
    wf = np.asarray(wf_tf).copy()
    M, bins = wf.shape
    hi = float(sk_threshold)
    lo = 2.0 - hi
    if lo > hi:
        lo, hi = hi, lo
    corr = (M - 1.0) / (M + 1.0)
    lo_, hi_ = lo * corr + 1.0, hi * corr + 1.0
    p = wf.real.astype(np.float64) ** 2 + wf.imag.astype(np.float64) ** 2
    s2 = p.sum(axis=0)
    s4 = (p * p).sum(axis=0)
    with np.errstate(divide="ignore", invalid="ignore"):
        sk = M * s4 / (s2 * s2)
    zap = (sk > hi_) | (sk < lo_) | (s2 == 0)
    wf[:, zap] = 0
    if normalize:
        mp = np.where(zap, 1.0, s2 / M)
        scale = np.where(zap, 0.0, 1.0 / np.sqrt(mp))
        wf = (wf * scale[None, :]).astype(wf.dtype)
    return wf


# ---------------------------------------------------------------------------
# Signal detection (reference: pipeline/signal_detect_pipe.hpp:252-441,
# signal_detect.hpp:25-70)
# ---------------------------------------------------------------------------


def zapped_channel_count(wf: np.ndarray) -> int:
    """Count channels whose FIRST time sample has zero power (zapped rows all
    start with 0; reference signal_detect_pipe.hpp:261-281 samples column 0
    via a stride-permutation iterator)."""
    wf = np.asarray(wf)
    col0 = wf[:, 0]
    p = col0.real.astype(np.float64) ** 2 + col0.imag.astype(np.float64) ** 2
    return int((p == 0).sum())


def time_series_sum(wf: np.ndarray, time_series_count: int,
                    dtype=np.float32) -> np.ndarray:
    """ts[j] = sum over channels of |wf[i][j]|^2, j < time_series_count
    (reference signal_detect_pipe.hpp:305-316).  float32 accumulation to match
    the GPU kernel."""
    wf = np.asarray(wf)
    p = (wf.real.astype(dtype)) ** 2 + (wf.imag.astype(dtype)) ** 2
    return p[:, :time_series_count].sum(axis=0, dtype=dtype)


def count_signal(ts: np.ndarray, snr_threshold: float) -> tuple[int, float]:
    """Threshold = snr * sqrt(mean(ts^2)) (ts assumed zero-mean), return
    (#above, threshold) (reference signal_detect.hpp:33-67)."""
    ts = np.asarray(ts, dtype=np.float64)
    thr = snr_threshold * np.sqrt((ts * ts).mean())
    return int((ts > thr).sum()), float(thr)


def boxcar_series(ts: np.ndarray, boxcar_length: int) -> np.ndarray:
    """box[i] = cumsum[i + L] - cumsum[i], inclusive scan with init 0
    (= sum of ts[i+1 .. i+L]); output length len(ts) - L
    (reference signal_detect_pipe.hpp:374-423)."""
    ts = np.asarray(ts)
    cum = np.cumsum(ts, dtype=np.float64)  # inclusive scan: cum[i] = sum ts[0..i]
    L = boxcar_length
    n = ts.size - L
    return (cum[L : L + n] - cum[0:n]).astype(ts.dtype)


def detect_signals(wf: np.ndarray, nsamps_reserved_real: int,
                   snr_threshold: float, channel_threshold: float,
                   max_boxcar_length: int) -> dict:
    """Full detection stage on a [n_channels][M] waterfall.

    Returns dict with 'time_series' (baseline-subtracted), 'zero_count', and
    'detections': list of (boxcar_length, signal_count, series) — boxcar 1 is
    the raw series.  Mirrors reference signal_detect_pipe_2.
    """
    wf = np.asarray(wf)
    n_channels, m = wf.shape
    zero_count = zapped_channel_count(wf)
    time_reserved = nsamps_reserved_real // n_channels
    ts_count = m if m <= time_reserved else m - time_reserved
    ts = time_series_sum(wf, ts_count)
    ts = (ts - ts.mean(dtype=np.float64)).astype(ts.dtype)

    detections = []
    if zero_count < channel_threshold * n_channels:
        cnt, thr = count_signal(ts, snr_threshold)
        if cnt > 0:
            detections.append((1, cnt, ts.copy()))
        L = 2
        while L <= max_boxcar_length and L < ts.size:
            box = boxcar_series(ts, L)
            cnt, thr = count_signal(box, snr_threshold)
            if cnt > 0:
                detections.append((L, cnt, box))
            L *= 2
    return {"time_series": ts, "zero_count": zero_count,
            "detections": detections}


# ---------------------------------------------------------------------------
# Filterbank output (no reference counterpart: its
# frequency_domain_filterbank_queue is a TODO; definition in
# docs/ARCHITECTURE.md, "Filterbank output")
# ---------------------------------------------------------------------------

FILTERBANK_QUANT_LEVEL = 64      # 8-bit level of a channel's mean
FILTERBANK_QUANT_PER_SIGMA = 16  # 8-bit levels per standard deviation


def filterbank_valid_rows(baseband_input_count: int,
                          spectrum_channel_count: int,
                          nsamps_reserved_real: int) -> int:
    """Waterfall time samples of a block that the next block does not repeat:
    V = (N - nsamps_reserved) / (2 S)."""
    return ((baseband_input_count - nsamps_reserved_real)
            // (2 * spectrum_channel_count))


def filterbank_block(wf: np.ndarray, valid_rows: int, tscrunch: int,
                     fscrunch: int, reverse: bool) -> np.ndarray:
    """Power plane P[R][C] (float64, time-major, channel fastest) of one
    [S][L] waterfall: R = valid_rows // tscrunch, C = S // fscrunch,
    P[r][c] = sum of |wf[row][t]|^2 over the cell's fscrunch rows and tscrunch
    time samples of the first ``valid_rows`` columns.  Output channel c holds
    rows c*fscrunch ... (reverse=False) or S-(c+1)*fscrunch ... (reverse=True,
    used for positive bandwidth so that channels run in descending
    frequency).  Zapped (all-zero) rows contribute 0 by themselves."""
    wf = np.asarray(wf)
    S, L = wf.shape
    if S % fscrunch != 0 or not 0 < tscrunch <= valid_rows <= L:
        raise ValueError("filterbank_block: bad geometry")
    R, C = valid_rows // tscrunch, S // fscrunch
    p = (wf.real.astype(np.float64) ** 2 + wf.imag.astype(np.float64) ** 2)
    p = p[:, :R * tscrunch].reshape(C, fscrunch, R, tscrunch).sum(axis=(1, 3))
    if reverse:
        p = p[::-1]
    return np.ascontiguousarray(p.T)


# polarization states of the two-polarization filterbank: name -> index as the
# kernel takes it (docs/ARCHITECTURE.md, "Polarization products")
POL_STATES = {"I": 0, "AABBCRCI": 1, "IQUV": 2}
POL_STATE_NIFS = {"I": 1, "AABBCRCI": 4, "IQUV": 4}


def pol_state_name(pol_state) -> str:
    """The state's name from a name or an index; ValueError otherwise."""
    if isinstance(pol_state, str):
        if pol_state in POL_STATES:
            return pol_state
    else:
        for name, index in POL_STATES.items():
            if index == pol_state:
                return name
    raise ValueError(f"unknown polarization state {pol_state!r} "
                     f"(one of {', '.join(POL_STATES)})")


def pol_products_block(wf_a: np.ndarray, wf_b: np.ndarray, valid_rows: int,
                       tscrunch: int, fscrunch: int, reverse: bool,
                       pol_state, flags_a=None, flags_b=None) -> np.ndarray:
    """Polarization products [R][P][C] (float64, channel fastest) of two
    [S][L] waterfalls A = x+iy, B = u+iv of the same sky, with R, C, the cell
    and the channel order of filterbank_block.  Per sample AA = x^2+y^2,
    BB = u^2+v^2, CR = xu+yv, CI = yu-xv, each summed over the cell.  A row
    whose flag is set in either ``flags_a`` or ``flags_b`` ([S], optional)
    contributes 0 to every product.  ``pol_state`` (name or index of
    POL_STATES): I -> AA+BB; AABBCRCI -> AA, BB, CR, CI; IQUV -> AA+BB, AA-BB,
    2 CR, 2 CI."""
    name = pol_state_name(pol_state)
    wf_a, wf_b = np.asarray(wf_a), np.asarray(wf_b)
    if wf_a.ndim != 2 or wf_a.shape != wf_b.shape:
        raise ValueError("pol_products_block: the waterfalls differ in shape")
    S, L = wf_a.shape
    if (tscrunch < 1 or fscrunch < 1 or S % fscrunch != 0
            or not tscrunch <= valid_rows <= L):
        raise ValueError("pol_products_block: bad geometry")
    keep = np.ones(S, dtype=bool)
    for flags in (flags_a, flags_b):
        if flags is not None:
            flags = np.asarray(flags)
            if flags.shape != (S,):
                raise ValueError("pol_products_block: flags must be [S]")
            keep &= flags == 0
    R, C = valid_rows // tscrunch, S // fscrunch
    x, y = wf_a.real.astype(np.float64), wf_a.imag.astype(np.float64)
    u, v = wf_b.real.astype(np.float64), wf_b.imag.astype(np.float64)

    def cells(p):
        p = np.where(keep[:, None], p, 0.0)
        p = p[:, :R * tscrunch].reshape(C, fscrunch, R, tscrunch)
        p = p.sum(axis=(1, 3))
        return p[::-1].T if reverse else p.T

    aa, bb = cells(x * x + y * y), cells(u * u + v * v)
    if name == "I":
        planes = [aa + bb]
    else:
        cr, ci = cells(x * u + y * v), cells(y * u - x * v)
        if name == "AABBCRCI":
            planes = [aa, bb, cr, ci]
        else:
            planes = [aa + bb, aa - bb, cr + cr, ci + ci]
    return np.ascontiguousarray(np.stack(planes, axis=1))


def filterbank_quantize(P: np.ndarray, mean: np.ndarray,
                        std: np.ndarray) -> np.ndarray:
    """q = clamp(rint((P - mean_c) * (16 / std_c) + 64), 0, 255) per channel
    (columns of P), 64 where std_c = 0; evaluated in float64."""
    P = np.asarray(P, dtype=np.float64)
    mean = np.asarray(mean, dtype=np.float64)
    std = np.asarray(std, dtype=np.float64)
    ok = std > 0
    scale = np.where(ok, FILTERBANK_QUANT_PER_SIGMA / np.where(ok, std, 1.0),
                     0.0)
    q = np.rint((P - mean[None, :]) * scale[None, :] + FILTERBANK_QUANT_LEVEL)
    q = np.where(ok[None, :], q, float(FILTERBANK_QUANT_LEVEL))
    return np.clip(q, 0, 255).astype(np.uint8)


def filterbank_channel_stats(P: np.ndarray) -> tuple[np.ndarray, np.ndarray]:
    """Per-channel mean and population standard deviation of P[R][C],
    accumulated in float64 and stored as float32."""
    P = np.asarray(P, dtype=np.float64)
    return P.mean(axis=0).astype(np.float32), P.std(axis=0).astype(np.float32)


def filterbank_header_fields(freq_low: float, bandwidth: float,
                             sample_rate: float, spectrum_channel_count: int,
                             tscrunch: int, fscrunch: int) -> dict:
    """fch1 / foff / tsamp / nchans of the filterbank file (channels in
    descending frequency, fch1 = centre of the highest channel)."""
    C = spectrum_channel_count // fscrunch
    bw = abs(bandwidth)
    return {
        "fch1": max(freq_low, freq_low + bandwidth) - bw / (2 * C),
        "foff": -bw / C,
        "nchans": C,
        "tsamp": 2.0 * spectrum_channel_count * tscrunch / sample_rate,
    }


# ---------------------------------------------------------------------------
# Pulsar folding (no reference counterpart; definition in
# docs/ARCHITECTURE.md, "Pulsar folding").  Phase is a wrapping 64-bit word,
# 2^64 = one turn; everything here is in Python integers and float64.
# ---------------------------------------------------------------------------

_TURN = 1 << 64
_WORD = _TURN - 1


def _turns_to_word(x: float) -> int:
    """x turns (0 <= x <= 1) as a phase word, rounded to nearest, 1 -> 0."""
    return round(math.ldexp(x, 64)) & _WORD


def fold_phase_step(sample_rate: float, f0: float) -> int:
    """Phase step per real sample: llrint(f0 / sample_rate * 2^64)."""
    return round(math.ldexp(f0 / sample_rate, 64))


def fold_check(spectrum_channel_count: int, sample_rate: float, f0: float,
               nbin: int) -> None:
    """The rejections shared by every layer."""
    if not 2 <= nbin <= 65536:
        raise ValueError("fold_nbin must be in 2..65536")
    if not f0 > 0 or not math.isfinite(f0):
        raise ValueError("fold_f0 (1 / fold_period) must be positive")
    if not f0 * (2 * spectrum_channel_count) / sample_rate < 1.0:
        raise ValueError("fold_f0 is too high: one waterfall sample "
                         "(2 * channels / sample_rate) must be shorter than "
                         "a period")


def fold_phase_words(n0: int, N: int, nsamps_reserved: int, S: int,
                     sample_rate: float, f0: float, f1: float,
                     phase0: float) -> tuple[int, int]:
    """(Phi_b, dPhi_b) of the block whose first real sample has index ``n0``
    in the stream: the phase word of waterfall column 0 and the step per
    column, at spin frequency f0 (Hz), derivative f1 (Hz/s) and phase0 turns
    at stream sample 0.  f0 * t is the integer product n0 * step, exact over
    any observation length; only the f1 terms go through float64."""
    step = fold_phase_step(sample_rate, f0)
    fresh = N - nsamps_reserved
    t0 = float(n0) / sample_rate
    t_mid = float(n0 + fresh // 2) / sample_rate
    p0 = phase0 - math.floor(phase0)
    q = 0.5 * f1 * t0 * t0
    phi = ((int(math.ldexp(p0, 64)) & _WORD) + n0 * step
           + _turns_to_word(q - math.floor(q))) & _WORD
    dphi = (2 * S * step
            + round(math.ldexp(f1 * t_mid * (float(2 * S) / sample_rate), 64))
            ) & _WORD
    return phi, dphi


def fold_bins(phi: int, dphi: int, V: int, nbin: int) -> np.ndarray:
    """bin(k) = (((phi + k * dphi) mod 2^64 >> 32) * nbin) >> 32, k < V."""
    return np.array([((((phi + k * dphi) & _WORD) >> 32) * nbin) >> 32
                     for k in range(V)], dtype=np.int64)


def fold_block(wf: np.ndarray, V: int, bins: np.ndarray, nbin: int,
               flags: np.ndarray | None = None
               ) -> tuple[np.ndarray, np.ndarray]:
    """(fold float64 [S][nbin], hits uint64 [nbin]) of one [S][L] waterfall:
    fold[c][b] = sum of |wf[c][k]|^2 over the k < V with bins[k] = b, rows
    with flags[c] != 0 contribute 0; hits[b] = number of such k."""
    wf = np.asarray(wf)
    S, L = wf.shape
    if not 0 < V <= L or len(bins) != V:
        raise ValueError("fold_block: bad geometry")
    p = (wf.real[:, :V].astype(np.float64) ** 2
         + wf.imag[:, :V].astype(np.float64) ** 2)
    if flags is not None:
        p[np.asarray(flags).astype(bool)] = 0.0
    fold = np.zeros((S, nbin), dtype=np.float64)
    np.add.at(fold.T, bins, p.T)
    hits = np.bincount(bins, minlength=nbin).astype(np.uint64)
    return fold, hits


class CpuFolder:
    """Accumulates blocks the way the engine does: a running stream position
    that advances by N - nsamps_reserved per block, fp64 profiles, u64 hits
    and weights."""

    def __init__(self, N: int, nsamps_reserved: int, S: int,
                 sample_rate: float, f0: float, f1: float, phase0: float,
                 nbin: int):
        fold_check(S, sample_rate, f0, nbin)
        if nsamps_reserved >= N or (N - nsamps_reserved) % (2 * S) != 0:
            raise ValueError("fold: baseband_input_count - nsamps_reserved "
                             "must be a positive multiple of 2 * channels")
        self.N, self.reserved, self.S = N, nsamps_reserved, S
        self.sample_rate, self.f0, self.f1 = sample_rate, f0, f1
        self.phase0, self.nbin = phase0, nbin
        self.V = (N - nsamps_reserved) // (2 * S)
        self.next_sample = 0
        self.reset()

    def reset(self) -> None:
        self.acc = np.zeros((self.S, self.nbin), dtype=np.float64)
        self.hits = np.zeros(self.nbin, dtype=np.uint64)
        self.weights = np.zeros(self.S, dtype=np.uint64)

    def add(self, wf: np.ndarray, flags: np.ndarray | None = None
            ) -> tuple[int, int, int]:
        """Fold one block at the running position; returns (n0, phi, dphi)."""
        n0 = self.next_sample
        phi, dphi = fold_phase_words(n0, self.N, self.reserved, self.S,
                                     self.sample_rate, self.f0, self.f1,
                                     self.phase0)
        bins = fold_bins(phi, dphi, self.V, self.nbin)
        fold, hits = fold_block(wf, self.V, bins, self.nbin, flags)
        self.acc += fold
        self.hits += hits
        good = (np.ones(self.S, dtype=bool) if flags is None
                else ~np.asarray(flags).astype(bool))
        self.weights += np.where(good, self.V, 0).astype(np.uint64)
        self.next_sample = n0 + self.N - self.reserved
        return n0, phi, dphi

    def read(self) -> tuple[np.ndarray, np.ndarray, np.ndarray]:
        return self.acc.copy(), self.hits.copy(), self.weights.copy()


# ---------------------------------------------------------------------------
# Incoherent DM-offset search on the filterbank power plane (no reference
# counterpart; definition in docs/ARCHITECTURE.md, "Incoherent DM-offset
# search")
# ---------------------------------------------------------------------------

INCOH_MAX_TRIALS = 1024
INCOH_MIN_ROWS = 2
INCOH_MAX_ROWS = 16384
INCOH_MAX_DELAY = 1 << 20
INCOH_MAX_WINDOW_BYTES = 1 << 30
INCOH_MAX_LENGTHS = 21


def incoherent_delays(fch1: float, foff: float, C: int, tsamp: float,
                      offsets) -> np.ndarray:
    """Delay table d[t][c] (int32, rows of the plane, all >= 0) of the offsets
    delta_t in pc cm^-3.  delta >= 0 delays channel c against channel 0 (the
    top of the band), delta < 0 against channel C - 1 (the bottom):
      delta >= 0: rint(D * delta   * (f(c)^-2     - f(0)^-2) / tsamp)
      delta <  0: rint(D * |delta| * (f(C-1)^-2   - f(c)^-2) / tsamp)
    with f(c) = fch1 + c * foff in MHz, every operation rounded in fp64 in the
    order written (the native table is the same bit for bit)."""
    offsets = np.atleast_1d(np.asarray(offsets, dtype=np.float64))
    if C < 1 or not tsamp > 0 or not np.all(np.isfinite(offsets)):
        raise ValueError("incoherent_delays: needs channels >= 1, tsamp > 0 "
                         "and finite offsets")
    f = np.float64(fch1) + np.arange(C, dtype=np.float64) * np.float64(foff)
    if not np.all(f > 0):
        raise ValueError("incoherent_delays: every channel centre must be "
                         "> 0 MHz")
    inv2 = 1.0 / (f * f)
    d = np.empty((offsets.size, C), dtype=np.float64)
    for t, delta in enumerate(offsets):
        diff = inv2 - inv2[0] if delta >= 0 else inv2[C - 1] - inv2
        d[t] = np.rint(D_DISPERSION * abs(delta) * diff / np.float64(tsamp))
    if d.size and (d.min() < 0 or d.max() > INCOH_MAX_DELAY):
        raise ValueError(f"incoherent_delays: delays of {d.min():.0f} .. "
                         f"{d.max():.0f} rows are outside 0 .. "
                         f"{INCOH_MAX_DELAY}")
    return d.astype(np.int32)


def incoherent_dedisperse(window: np.ndarray, delays: np.ndarray,
                          R: int) -> np.ndarray:
    """Y[t][j] = sum_c window[j + delays[t][c]][c], j < R, in float64.
    window: [D + R][C] with every delay in 0 .. D."""
    window = np.asarray(window, dtype=np.float64)
    delays = np.asarray(delays)
    T, C = delays.shape
    if window.ndim != 2 or window.shape[1] != C or not 1 <= R <= len(window):
        raise ValueError("incoherent_dedisperse: bad geometry")
    if delays.min() < 0 or delays.max() > len(window) - R:
        raise ValueError("incoherent_dedisperse: a delay is outside the window")
    rows = np.arange(R)[:, None]
    cols = np.arange(C)[None, :]
    Y = np.empty((T, R), dtype=np.float64)
    for t in range(T):
        Y[t] = window[rows + delays[t][None, :], cols].sum(axis=1)
    return Y


def incoherent_lengths(max_boxcar: int) -> list[int]:
    """Boxcar lengths 1, 2, 4 ... <= max_boxcar (at most INCOH_MAX_LENGTHS)."""
    out, l = [], 1
    while l <= max_boxcar and len(out) < INCOH_MAX_LENGTHS:
        out.append(l)
        l *= 2
    return out


def incoherent_series(y: np.ndarray, length: int) -> tuple[float, np.ndarray]:
    """(mu, b_l) of one row: z = y - mu; length 1 is z itself, length l >= 2
    is cs[i + l] - cs[i], i + l < R, cs the inclusive scan of z.  Empty where
    the length has no window."""
    y = np.asarray(y, dtype=np.float64)
    mu = y.sum() / y.size
    z = y - mu
    if length == 1:
        return mu, z
    cs = np.cumsum(z)
    n = max(y.size - length, 0)
    return mu, cs[length:length + n] - cs[:n]


def incoherent_detect(Y: np.ndarray, snr: float, max_boxcar: int) -> dict:
    """Per trial (row of Y) and boxcar length, all float64: 'peak' and 'index'
    (lowest index attaining it), 'rms' = sqrt(sum b^2 / n), 'count' = #{b > snr
    * rms}, 'snr' = peak / rms (0 where rms = 0), each [T][NL]; 'mu' [T];
    'lengths'.  A length without a window has peak -inf, index -1, rms 0,
    count 0."""
    Y = np.asarray(Y, dtype=np.float64)
    T, R = Y.shape
    lengths = incoherent_lengths(max_boxcar)
    NL = len(lengths)
    out = {
        "lengths": lengths,
        "peak": np.full((T, NL), -np.inf),
        "index": np.full((T, NL), -1, dtype=np.int64),
        "rms": np.zeros((T, NL)),
        "count": np.zeros((T, NL), dtype=np.int64),
        "snr": np.zeros((T, NL)),
        "mu": np.zeros(T),
    }
    for t in range(T):
        for k, l in enumerate(lengths):
            mu, b = incoherent_series(Y[t], l)
            out["mu"][t] = mu
            if b.size == 0:
                continue
            rms = np.sqrt((b * b).sum() / b.size)
            i = int(np.argmax(b))  # first occurrence
            out["peak"][t, k] = b[i]
            out["index"][t, k] = i
            out["rms"][t, k] = rms
            out["count"][t, k] = int((b > snr * rms).sum())
            out["snr"][t, k] = b[i] / rms if rms > 0 else 0.0
    return out


def incoherent_result_trials(det: dict, offsets) -> list[dict]:
    """The detect arrays in the per-trial form IncoherentSearch.wait returns."""
    trials = []
    for t, delta in enumerate(offsets):
        trials.append({
            "offset": float(delta), "mean": float(det["mu"][t]),
            "lengths": [{
                "boxcar_length": int(l), "peak": float(det["peak"][t, k]),
                "index": int(det["index"][t, k]),
                "rms": float(det["rms"][t, k]),
                "count": int(det["count"][t, k]),
                "snr": float(det["snr"][t, k]),
            } for k, l in enumerate(det["lengths"])]})
    return trials


INCOH_NORM_MAX_BLOCKS = 65536


def incoherent_norm_stats(P: np.ndarray) -> tuple[np.ndarray, np.ndarray]:
    """(m, v) per channel of one block plane [R][C], float64: the mean and the
    population variance, from the sums of x - x0 and (x - x0)^2 with
    x0 = P[0][c], so a constant channel has exactly v = 0."""
    P = np.asarray(P, dtype=np.float64)
    if P.ndim != 2 or P.shape[0] < 1 or P.shape[1] < 1:
        raise ValueError("incoherent_norm_stats: needs a plane [R][C]")
    R = np.float64(P.shape[0])
    d = P - P[0]
    ds = d.sum(axis=0) / R
    v = (d * d).sum(axis=0) / R - ds * ds
    return P[0] + ds, np.maximum(v, 0.0)


def incoherent_norm_gain(V: np.ndarray) -> np.ndarray:
    """G = (float32)(1 / sqrt(V)) where V > 0, else 0."""
    V = np.asarray(V, dtype=np.float64)
    G = np.zeros(V.shape, dtype=np.float32)
    live = V > 0
    G[live] = (1.0 / np.sqrt(V[live])).astype(np.float32)
    return G


def incoherent_norm_apply(P: np.ndarray, M: np.ndarray,
                          G: np.ndarray) -> np.ndarray:
    """(P - (float32)M) * G in float32, each operation rounded on its own."""
    P = np.asarray(P, dtype=np.float32)
    m32 = np.asarray(M, dtype=np.float64).astype(np.float32)
    return (P - m32[None, :]) * np.asarray(G, dtype=np.float32)[None, :]


class CpuIncoherentSearch:
    """Streaming search with the history, priming and result semantics of the
    native IncoherentSearch: block b's output row j stands for global row
    b * R - D_max + j, rows before the stream are zero, and a block is valid
    (and searched) iff b * R >= D_max.  With normalize, a block's rows enter
    the history as (x - M) * G of the running per-channel state, which block
    b updates with alpha = 1 / min(b + 1, normalize_blocks) before it is
    applied to block b."""

    def __init__(self, R: int, C: int, fch1: float, foff: float, tsamp: float,
                 offsets, snr_threshold: float, max_boxcar: int,
                 normalize: bool = False, normalize_blocks: int = 8):
        self.normalize = bool(normalize)
        self.normalize_blocks = int(normalize_blocks)
        if not 1 <= self.normalize_blocks <= INCOH_NORM_MAX_BLOCKS:
            raise ValueError(f"incoherent search: normalize_blocks must be "
                             f"1 .. {INCOH_NORM_MAX_BLOCKS}")
        self.offsets = [float(x) for x in np.atleast_1d(offsets)]
        if not 1 <= len(self.offsets) <= INCOH_MAX_TRIALS:
            raise ValueError(f"incoherent search: needs 1 .. "
                             f"{INCOH_MAX_TRIALS} offsets")
        if not INCOH_MIN_ROWS <= R <= INCOH_MAX_ROWS:
            raise ValueError(f"incoherent search: rows per block must be "
                             f"{INCOH_MIN_ROWS} .. {INCOH_MAX_ROWS}")
        if C < 1 or max_boxcar < 1:
            raise ValueError("incoherent search: needs channels >= 1 and "
                             "max_boxcar >= 1")
        self.R, self.C = int(R), int(C)
        self.snr_threshold, self.max_boxcar = float(snr_threshold), max_boxcar
        self.delays = incoherent_delays(fch1, foff, C, tsamp, self.offsets)
        self.d_max = int(self.delays.max())
        if (self.d_max + R) * C * 4 > INCOH_MAX_WINDOW_BYTES:
            raise ValueError(
                f"incoherent search: the history of (D_max + R) * C * 4 bytes "
                f"(D_max = {self.d_max} rows) exceeds the cap of "
                f"{INCOH_MAX_WINDOW_BYTES}")
        self.reset()

    def reset(self) -> None:
        self.window = np.zeros((self.d_max + self.R, self.C), dtype=np.float64)
        self.block = 0
        self.M = np.zeros(self.C, dtype=np.float64)
        self.V = np.zeros(self.C, dtype=np.float64)
        self.G = np.zeros(self.C, dtype=np.float32)

    def add(self, plane: np.ndarray) -> dict:
        """One block's [R][C] plane -> {'valid', 'first_row', 'block',
        'live_channels' (0 unless normalize), 'Y' (float64 [T][R]), 'trials'
        (empty unless valid)}."""
        plane = np.asarray(plane, dtype=np.float64)
        if plane.shape != (self.R, self.C):
            raise ValueError("incoherent search: plane shape differs")
        b = self.block
        live = 0
        if self.normalize:
            alpha = np.float64(1.0) / np.float64(
                min(b + 1, self.normalize_blocks))
            m, v = incoherent_norm_stats(plane)
            self.M = self.M + alpha * (m - self.M)
            self.V = self.V + alpha * (v - self.V)
            self.G = incoherent_norm_gain(self.V)
            live = int((self.G > 0).sum())
            plane = incoherent_norm_apply(plane, self.M, self.G).astype(
                np.float64)
        self.window = np.concatenate([self.window[self.R:], plane])
        self.block += 1
        Y = incoherent_dedisperse(self.window, self.delays, self.R)
        valid = b * self.R >= self.d_max
        trials = []
        if valid:
            trials = incoherent_result_trials(
                incoherent_detect(Y, self.snr_threshold, self.max_boxcar),
                self.offsets)
        return {"valid": valid, "first_row": b * self.R - self.d_max,
                "block": b, "live_channels": live, "Y": Y, "trials": trials}


def incoherent_candidate_lines(result: dict, tsamp: float, dm: float) -> list[str]:
    """Candidate lines of one valid block's result, one per (trial, length)
    with count > 0: block ordinal, time of the peak in seconds from the start
    of the stream ((first_row + index) * tsamp), dm + delta, boxcar length,
    snr.  The native backend prints the same bytes."""
    lines = []
    if not result["valid"]:
        return lines
    for tr in result["trials"]:
        for ln in tr["lengths"]:
            if ln["count"] > 0:
                time_s = (result["first_row"] + ln["index"]) * tsamp
                lines.append("%d %.9f %.6f %d %.6f\n" % (
                    result["block"], time_s, dm + tr["offset"],
                    ln["boxcar_length"], ln["snr"]))
    return lines


# ---------------------------------------------------------------------------
# Spectrum simplification for display
# (reference: spectrum/simplify_spectrum.hpp:37-731)
# ---------------------------------------------------------------------------


def resample_power_2d(wf_power: np.ndarray, out_h: int, out_w: int) -> np.ndarray:
    """Area-averaged resample of a [n_channels][M] power waterfall to
    [out_h][out_w] — the capability of resample_spectrum_3 (v2 math: full
    average over the covered source region with fractional edge coverage,
    simplify_spectrum.hpp:276-620)."""
    src = np.asarray(wf_power, dtype=np.float64)
    h, w = src.shape

    def overlap_matrix(n_out, n_in):
        # W[o, i] = length of overlap between out-cell o (width n_in/n_out in
        # source units) and source cell i, normalized so each row sums to 1.
        W = np.zeros((n_out, n_in))
        step = n_in / n_out
        for o in range(n_out):
            a, b = o * step, (o + 1) * step
            i0, i1 = int(np.floor(a)), int(np.ceil(b))
            for i in range(i0, min(i1, n_in)):
                W[o, i] = max(0.0, min(b, i + 1) - max(a, i))
            W[o] /= step
        return W

    return overlap_matrix(out_h, h) @ src @ overlap_matrix(out_w, w).T


def normalize_by_mean(img: np.ndarray) -> np.ndarray:
    """x *= 1 / (2 * mean) (reference simplify_spectrum.hpp:627-644)."""
    img = np.asarray(img, dtype=np.float64)
    m = img.mean()
    if m == 0:
        return img
    return img / (2.0 * m)


# GUI colors (reference config.hpp:60-68)
COLOR_0 = 0xFF1F1E33
COLOR_1 = 0xFF33E1F1
COLOR_OVERFLOW = 0xFFE0E1CC


def generate_pixmap(intensity: np.ndarray) -> np.ndarray:
    """intensity in [0,1] → ARGB32 via per-channel lerp between COLOR_0 and
    COLOR_1; out-of-range → COLOR_OVERFLOW (reference simplify_spectrum.hpp:700-731).

    Rounding rule, shared with the HIP kernel (csrc/include/srtb_kernels.h):
    each channel is c0 + (c1 - c0) * x rounded to the nearest integer, ties
    away from zero (C's roundf, not NumPy's ties-to-even round; the reference
    truncates).  In range means 0 <= x <= 1: -0.0 is in range, NaN and
    infinities are not."""
    x = np.asarray(intensity, dtype=np.float64)
    out = np.empty(x.shape, dtype=np.uint32)
    ok = (x >= 0) & (x <= 1)
    x = np.where(ok, x, 0.0)

    def chan(c0, c1):
        # the value is in [0, 255], where away from zero is floor(v + 1/2);
        # float64 holds v exactly for any float32 x large enough to bring it
        # near a half-integer
        v = c0 + (c1 - c0) * x
        return np.clip(np.floor(v + 0.5), 0, 255).astype(np.uint32)

    a = chan((COLOR_0 >> 24) & 0xFF, (COLOR_1 >> 24) & 0xFF)
    r = chan((COLOR_0 >> 16) & 0xFF, (COLOR_1 >> 16) & 0xFF)
    g = chan((COLOR_0 >> 8) & 0xFF, (COLOR_1 >> 8) & 0xFF)
    b = chan(COLOR_0 & 0xFF, COLOR_1 & 0xFF)
    out[:] = (a << 24) | (r << 16) | (g << 8) | b
    out[~ok] = COLOR_OVERFLOW
    return out


# ---------------------------------------------------------------------------
# Misc device algorithms
# ---------------------------------------------------------------------------


def running_mean_init_average(data: np.ndarray, windowsize: int) -> np.ndarray:
    """Per-channel mean of the first ``windowsize`` time samples of a
    time-major [nsamp][nchan] array (reference algorithm/running_mean.hpp:61-77)."""
    x = np.asarray(data, dtype=np.float64)
    return x[:windowsize, :].sum(axis=0) / windowsize


def running_mean(data: np.ndarray, windowsize: int,
                 ave: np.ndarray) -> tuple[np.ndarray, np.ndarray]:
    """1-bit threshold of a time-major [nsamp][nchan] array against a
    sliding-window running mean (reference algorithm/running_mean.hpp:31-59).

    out[t][j] = (data[t][j] > ave_j) where ave_j slides forward by
    (data[t+window][j] - data[t][j]) / window; the last ``window`` outputs
    update the mean from a mirrored tail.  Returns (out, updated_ave).
    """
    x = np.asarray(data, dtype=np.float64)
    nsamp, nchan = x.shape
    out = np.zeros((nsamp, nchan), dtype=np.uint8)
    ave = np.asarray(ave, dtype=np.float64).copy()
    for j in range(nchan):
        a = ave[j]
        for i in range(windowsize, nsamp):
            head = x[i - windowsize, j]
            tail = x[i, j]
            out[i - windowsize, j] = 1 if head > a else 0
            a += (tail - head) / windowsize
        for i in range(windowsize):
            head = x[nsamp + i - windowsize, j]
            tail = x[nsamp - i - 1, j]
            out[i + nsamp - windowsize, j] = 1 if head > a else 0
            a += (tail - head) / windowsize
        ave[j] = a
    return out, ave


def correlate_spectra(f1: np.ndarray, f2: np.ndarray, scale: float) -> np.ndarray:
    """corr[i] = scale * f1[i] * conj(f2[i]) (reference src/correlator.cpp:116-119)."""
    f1 = np.asarray(f1)
    f2 = np.asarray(f2)
    return (scale * f1 * np.conj(f2)).astype(f1.dtype)
