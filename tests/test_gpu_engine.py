"""GPU end-to-end tests: native PipelineEngine vs the CPU oracle pipeline."""

import numpy as np
import pytest
import torch

from srtb_amd import ref
from srtb_amd.config import Config
from srtb_amd.pipeline.cpu import CpuPipeline, synthesize_dispersed_pulse

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def C():
    from srtb_amd.ops import native
    torch.cuda.set_device(0)
    return native()


def small_cfg(bits=-8, dm=60.0):
    c = Config()
    c.baseband_input_count = 1 << 18
    c.spectrum_channel_count = 1 << 6
    c.baseband_input_bits = bits
    c.baseband_freq_low = 1400.0
    c.baseband_bandwidth = 64.0
    c.baseband_sample_rate = 128e6
    c.dm = dm
    c.mitigate_rfi_average_method_threshold = 1e30
    c.mitigate_rfi_spectral_kurtosis_threshold = 1e30
    c.signal_detect_signal_noise_threshold = 6.0
    c.signal_detect_max_boxcar_length = 16
    return c


def make_engine(C, cfg, **kw):
    pipe = CpuPipeline(cfg)
    args = dict(
        n=cfg.baseband_input_count, nbits=cfg.baseband_input_bits,
        channels=cfg.spectrum_channel_count, freq_low=cfg.baseband_freq_low,
        bandwidth=cfg.baseband_bandwidth, sample_rate=cfg.baseband_sample_rate,
        dm=cfg.dm, rfi_threshold=cfg.mitigate_rfi_average_method_threshold,
        sk_threshold=cfg.mitigate_rfi_spectral_kurtosis_threshold,
        snr_threshold=cfg.signal_detect_signal_noise_threshold,
        max_boxcar=cfg.signal_detect_max_boxcar_length,
        nsamps_reserved=pipe.nsamps_reserved(), zap_ranges=[],
        use_phase_table=False, enable_rfi_s1=True, enable_sk=True, n_slots=2)
    args.update(kw)
    return C.PipelineEngine(**args)


@pytest.mark.parametrize("n,s,fft", [(1 << 18, 1 << 6, 0),
                                      (1 << 20, 1 << 6, 0),
                                      (1 << 18, 1 << 6, 1),
                                      (1 << 20, 1 << 6, 2)])
def test_engine_matches_cpu_oracle(C, n, s, fft):
    """Shape 2 has waterfall len 2^13 > 4096 → exercises the multi-pass
    native FFT with the RFI+dedispersion preop fused into its first column
    pass; variant 3 runs the hipFFT fallback backend; variant 4 runs the
    auto backend, whose small waterfall length (8192) picks the mixed
    native-forward + rocFFT-backward path."""
    cfg = small_cfg()
    cfg.baseband_input_count = n
    cfg.spectrum_channel_count = s
    # enable real thresholds so RFI/SK paths execute
    cfg.mitigate_rfi_average_method_threshold = 20.0
    cfg.mitigate_rfi_spectral_kurtosis_threshold = 1.5
    rng = np.random.default_rng(0)
    raw = np.clip(np.round(rng.normal(0, 16, cfg.baseband_input_count)),
                  -128, 127).astype(np.int8).view(np.uint8)

    res_cpu = CpuPipeline(cfg).process_block(raw)
    eng = make_engine(C, cfg,
                      rfi_threshold=cfg.mitigate_rfi_average_method_threshold,
                      sk_threshold=cfg.mitigate_rfi_spectral_kurtosis_threshold,
                      fft_backend=fft)
    slot = eng.submit(torch.from_numpy(raw.copy()))
    res = eng.wait(slot)

    ts_gpu = eng.time_series(slot).cpu().numpy()
    ts_cpu = res_cpu["time_series"]
    assert ts_gpu.shape == ts_cpu.shape
    scale = max(np.abs(ts_cpu).max(), 1e-9)
    np.testing.assert_allclose(ts_gpu / scale, ts_cpu / scale, atol=2e-3)

    wf_gpu = eng.waterfall(slot).cpu().numpy()
    wf_cpu = res_cpu["waterfall"]
    wscale = max(np.abs(wf_cpu).max(), 1e-9)
    np.testing.assert_allclose(wf_gpu / wscale, wf_cpu / wscale, atol=5e-3)

    assert res["zero_count"] == res_cpu["zero_count"]


def test_engine_detects_dispersed_pulse(C):
    cfg = small_cfg()
    pipe = CpuPipeline(cfg)
    t_pulse = 0.4 * cfg.baseband_input_count / cfg.baseband_sample_rate
    raw = synthesize_dispersed_pulse(cfg, t_pulse, pulse_amp=40.0,
                                     noise_sigma=2.0)
    eng = make_engine(C, cfg)
    slot = eng.submit(torch.from_numpy(raw.copy()))
    res = eng.wait(slot)
    counts = dict(res["counts"])
    assert counts[1] > 0, f"pulse not detected: {res}"
    ts = eng.time_series(slot).cpu().numpy()
    expect_bin = int(t_pulse * cfg.baseband_sample_rate) // (
        2 * cfg.spectrum_channel_count)
    assert abs(int(np.argmax(ts)) - expect_bin) <= 2


def test_engine_quiet_on_noise(C):
    cfg = small_cfg()
    cfg.signal_detect_signal_noise_threshold = 8.0
    rng = np.random.default_rng(3)
    raw = np.clip(np.round(rng.normal(0, 16, cfg.baseband_input_count)),
                  -128, 127).astype(np.int8).view(np.uint8)
    eng = make_engine(C, cfg, snr_threshold=8.0)
    slot = eng.submit(torch.from_numpy(raw.copy()))
    res = eng.wait(slot)
    assert all(c == 0 for _, c in res["counts"]), res


@pytest.mark.parametrize("bits", [1, 2, 4])
def test_engine_subbyte_paths(C, bits):
    """Sub-byte formats run with the unpack fused into the forward FFT's
    first column pass (decode-at-load); the dispersed pulse must still land
    in the right time-series bin."""
    cfg = small_cfg(bits=bits)
    t_pulse = 0.5 * cfg.baseband_input_count / cfg.baseband_sample_rate
    raw = synthesize_dispersed_pulse(cfg, t_pulse, pulse_amp=12.0,
                                     noise_sigma=2.0)
    eng = make_engine(C, cfg)
    slot = eng.submit(torch.from_numpy(raw.copy()))
    eng.wait(slot)
    ts = eng.time_series(slot).cpu().numpy()
    expect_bin = int(t_pulse * cfg.baseband_sample_rate) // (
        2 * cfg.spectrum_channel_count)
    assert abs(int(np.argmax(ts)) - expect_bin) <= 2


@pytest.mark.parametrize("bits", [1, 2, 4, 8, -8, 16, -16])
def test_engine_subbyte_fused_matches_unfused(C, monkeypatch, bits):
    """The fused decode-at-load path must produce the same time series as
    the standalone unpack kernel path (SRTB_NO_FUSED_UNPACK)."""
    cfg = small_cfg(bits=bits)
    rng = np.random.default_rng(7)
    nbytes = cfg.baseband_input_count * abs(bits) // 8
    raw = rng.integers(0, 256, nbytes, dtype=np.uint8)
    eng = make_engine(C, cfg)
    slot = eng.submit(torch.from_numpy(raw.copy()))
    eng.wait(slot)
    ts_fused = eng.time_series(slot).cpu().numpy().copy()
    monkeypatch.setenv("SRTB_NO_FUSED_UNPACK", "1")
    eng2 = make_engine(C, cfg)
    slot2 = eng2.submit(torch.from_numpy(raw.copy()))
    eng2.wait(slot2)
    ts_plain = eng2.time_series(slot2).cpu().numpy()
    np.testing.assert_allclose(ts_fused, ts_plain, rtol=1e-5, atol=1e-3)


def test_engine_double_buffering_order(C):
    """Submitting several blocks through both slots returns per-block results."""
    cfg = small_cfg()
    eng = make_engine(C, cfg)
    rng = np.random.default_rng(4)
    peaks = []
    raws = []
    for i in range(4):
        raw = np.clip(np.round(rng.normal(0, 16, cfg.baseband_input_count)),
                      -128, 127).astype(np.int8).view(np.uint8)
        raws.append(torch.from_numpy(raw.copy()))
    slots = []
    for r in raws:
        slots.append(eng.submit(r))
    eng.synchronize()
    assert slots == [0, 1, 0, 1]


def test_engine_boxcar_series_readback(C):
    cfg = small_cfg()
    eng = make_engine(C, cfg)
    rng = np.random.default_rng(5)
    raw = np.clip(np.round(rng.normal(0, 16, cfg.baseband_input_count)),
                  -128, 127).astype(np.int8).view(np.uint8)
    slot = eng.submit(torch.from_numpy(raw.copy()))
    eng.wait(slot)
    ts = eng.time_series(slot).cpu().numpy()
    box = eng.boxcar_series(slot, 4).cpu().numpy()
    expect = ref.boxcar_series(ts, 4)
    np.testing.assert_allclose(box, expect, rtol=1e-3, atol=2e-2)


def test_engine_fused_window(C):
    """window_kind=2 (hamming) fused at unpack matches the CPU oracle with
    the same window."""
    cfg = small_cfg()
    rng = np.random.default_rng(9)
    raw = np.clip(np.round(rng.normal(0, 16, cfg.baseband_input_count)),
                  -128, 127).astype(np.int8).view(np.uint8)
    pipe = CpuPipeline(cfg)
    pipe.window_kind = "hamming"
    res_cpu = pipe.process_block(raw)
    eng = make_engine(C, cfg, window_kind=2)
    slot = eng.submit(torch.from_numpy(raw.copy()))
    eng.wait(slot)
    ts_gpu = eng.time_series(slot).cpu().numpy()
    ts_cpu = res_cpu["time_series"]
    scale = max(np.abs(ts_cpu).max(), 1e-9)
    np.testing.assert_allclose(ts_gpu / scale, ts_cpu / scale, atol=2e-3)


def test_engine_boxcar_ladder_matches_numpy(C):
    """The fused boxcar ladder's per-length thresholds and counts must match
    a NumPy recomputation from the engine's own time series."""
    cfg = small_cfg()
    rng = np.random.default_rng(3)
    raw = np.clip(np.round(rng.normal(0, 16, cfg.baseband_input_count)),
                  -128, 127).astype(np.int8).view(np.uint8)
    eng = make_engine(C, cfg, snr_threshold=3.0)  # low snr → nonzero counts
    slot = eng.submit(torch.from_numpy(raw.copy()))
    res = eng.wait(slot)
    ts = eng.time_series(slot).cpu().numpy().astype(np.float64)
    cum = np.cumsum(ts)
    snr = 3.0
    assert len(res["counts"]) >= 3
    for (L, cnt), thr in zip(res["counts"][1:], res["thresholds"][1:]):
        box = cum[L:] - cum[:-L]
        thr_exp = snr * np.sqrt(np.mean(box * box))
        assert abs(thr - thr_exp) / thr_exp < 1e-3, (L, thr, thr_exp)
        cnt_exp = int((box > thr_exp).sum())
        # fp32 cumsum vs fp64 recompute can flip borderline samples
        assert abs(cnt - cnt_exp) <= max(3, 0.02 * max(cnt_exp, 1)), \
            (L, cnt, cnt_exp)


def test_engine_watfft_window_deapply(C):
    """K21: with a non-rectangle window the waterfall is divided by the
    length-L window after the backward FFT (reference fft_pipe.hpp:350-358).
    Compare the engine waterfall against the CPU oracle with and without
    the window — the two must differ exactly by the de-apply+window chain."""
    cfg = small_cfg(dm=0.0)
    rng = np.random.default_rng(23)
    raw = np.clip(np.round(rng.normal(0, 16, cfg.baseband_input_count)),
                  -128, 127).astype(np.int8).view(np.uint8)
    pipe = CpuPipeline(cfg)
    pipe.window_kind = "hamming"
    res_cpu = pipe.process_block(raw)
    eng = make_engine(C, cfg, window_kind=2)
    slot = eng.submit(torch.from_numpy(raw.copy()))
    eng.wait(slot)
    wf_gpu = eng.waterfall(slot).cpu().numpy()
    wf_cpu = res_cpu["waterfall"].astype(np.complex64)
    scale = max(np.abs(wf_cpu).max(), 1e-9)
    np.testing.assert_allclose(wf_gpu / scale, wf_cpu / scale, atol=2e-3)
    # sanity: the de-apply actually changed the waterfall (window != rect)
    pipe2 = CpuPipeline(cfg)
    res_rect = pipe2.process_block(raw)
    assert not np.allclose(wf_cpu / scale,
                           res_rect["waterfall"].astype(np.complex64) / scale,
                           atol=2e-3)


def test_engine_hip_graph_replay(C):
    """Graph-captured replay produces identical results to direct enqueue."""
    cfg = small_cfg()
    rng = np.random.default_rng(11)
    raw_np = np.clip(np.round(rng.normal(0, 16, cfg.baseband_input_count)),
                     -128, 127).astype(np.int8).view(np.uint8)
    raw = torch.from_numpy(raw_np.copy()).pin_memory()
    eng_a = make_engine(C, cfg)
    eng_b = make_engine(C, cfg, use_hip_graph=True)
    ts_ref = None
    for i in range(5):  # submissions 3+ replay the captured graph
        sa = eng_a.submit(raw)
        ra = eng_a.wait(sa)
        sb = eng_b.submit(raw)
        rb = eng_b.wait(sb)
        assert ra["counts"] == rb["counts"], (i, ra, rb)
        assert ra["zero_count"] == rb["zero_count"]
        ta = eng_a.time_series(sa).cpu().numpy()
        tb = eng_b.time_series(sb).cpu().numpy()
        np.testing.assert_array_equal(ta, tb)
