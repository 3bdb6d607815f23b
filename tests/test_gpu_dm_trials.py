"""GPU tests of the shared-spectrum DM-trial search: one forward half per
block, one backward half per trial (engine submit_trials), the out-of-place
RFI+dedispersion kernel and the peak kernel.

Yardstick for numerics: a separate engine built with max_dm_trials=0 and fed
the same raw block through submit(raw, dm_override=dm) — the single-DM chain.
Both sides run the same kernels on identical inputs, so equality is bitwise.
"""

import os
import subprocess

import numpy as np
import pytest
import torch

from srtb_amd.config import Config
from srtb_amd.pipeline.cpu import synthesize_dispersed_pulse

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "bin", "srtb-backend")

DMS = [0.0, 60.0, 25.0, 60.0]
ZAP = [[100, 300]]


@pytest.fixture(scope="module")
def C():
    from srtb_amd.ops import native
    torch.cuda.set_device(0)
    return native()


def make_engine(C, n=1 << 18, s=1 << 6, fft=0, nbits=-8, **kw):
    args = dict(
        n=n, nbits=nbits, channels=s, freq_low=1400.0, bandwidth=64.0,
        sample_rate=128e6, dm=60.0, rfi_threshold=20.0, sk_threshold=1.5,
        snr_threshold=6.0, max_boxcar=16, nsamps_reserved=0, zap_ranges=ZAP,
        use_phase_table=False, enable_rfi_s1=True, enable_sk=True, n_slots=2,
        fft_backend=fft)
    args.update(kw)
    return C.PipelineEngine(**args)


def noise_block(n, seed):
    rng = np.random.default_rng(seed)
    raw = np.clip(np.round(rng.normal(0, 16, n)), -128, 127)
    return torch.from_numpy(raw.astype(np.int8).view(np.uint8).copy())


def yardstick(C, raw, dms, **kw):
    """Single-DM chain per trial on an engine without the feature."""
    eng = make_engine(C, **kw)
    out = []
    for dm in dms:
        slot = eng.submit(raw, dm_override=dm)
        res = eng.wait(slot)
        out.append(dict(res=res, ts=eng.time_series(slot).clone(),
                        wf=eng.waterfall(slot).clone()))
    return out


# ---- 1. trials equal the single-DM path ----

@pytest.mark.parametrize("n,s,fft", [
    (1 << 18, 1 << 6, 0),   # native single-pass backward: out-of-place kernel
    (1 << 20, 1 << 6, 0),   # waterfall 2^13: fused column pre-op, first_pass_out
    (1 << 20, 1 << 6, 2),   # native forward, rocFFT backward
    (1 << 18, 1 << 6, 1),   # hipFFT throughout
])
def test_trials_equal_single_dm_path(C, n, s, fft):
    """dm 0 takes the column-polynomial phase on the fused path, 60 the
    per-bin phase; the repeated 60 fails if a trial damaged the retained
    spectrum."""
    raw = noise_block(n, 0)
    want = yardstick(C, raw, DMS, n=n, s=s, fft=fft)
    eng = make_engine(C, n=n, s=s, fft=fft, max_dm_trials=len(DMS))
    slot = eng.submit_trials(raw, DMS)
    got = eng.wait_trials(slot)
    plane = eng.dm_time_plane(slot)
    assert len(got) == len(DMS)
    assert tuple(plane.shape) == (len(DMS), eng.ts_count)
    for k, dm in enumerate(DMS):
        w = want[k]
        assert got[k]["dm"] == dm
        assert torch.equal(plane[k], w["ts"]), (k, dm)
        assert got[k]["counts"] == w["res"]["counts"], (k, dm)
        assert got[k]["thresholds"] == w["res"]["thresholds"], (k, dm)
        assert got[k]["zero_count"] == w["res"]["zero_count"], (k, dm)
    for k in [1, 0, 3, 2]:
        eng.select_trial(slot, k)
        assert torch.equal(eng.waterfall(slot), want[k]["wf"]), k
        assert torch.equal(eng.time_series(slot), want[k]["ts"]), k
        # the re-run rewrote the same rows
        assert torch.equal(plane[k], want[k]["ts"]), k
    # generic callers: wait() reports the trial most recently run
    assert eng.wait(slot)["counts"] == want[2]["res"]["counts"]


# ---- 2. out-of-place RFI + dedispersion kernel ----

@pytest.mark.parametrize("nc", [1, 255, (1 << 17) + 3])
@pytest.mark.parametrize("rfi", [False, True])
def test_rfi_dedisperse_fused_out_of_place(C, nc, rfi):
    g = torch.Generator().manual_seed(nc)
    spec = torch.view_as_complex(torch.randn(nc, 2, generator=g)).cuda()
    keep = spec.clone()
    ranges = [[0, 3], [100, 120]]
    args = (rfi, 3.0, 64, ranges, 1400.0, 1464.0, 64.0 / nc, 60.0)

    inplace = spec.clone()
    C.rfi_dedisperse_fused(inplace, *args)
    assert not torch.equal(inplace, keep)

    out = torch.full_like(spec, float("nan"))
    C.rfi_dedisperse_fused(spec, *args, out=out)
    assert torch.equal(torch.view_as_real(out), torch.view_as_real(inplace))
    assert torch.equal(torch.view_as_real(spec), torch.view_as_real(keep))

    alias = spec.clone()
    C.rfi_dedisperse_fused(alias, *args, out=alias)
    assert torch.equal(torch.view_as_real(alias), torch.view_as_real(inplace))


# ---- 3. detect_peaks against numpy ----

LADDER = [2, 4, 8, 16]


def check_peaks(C, ts, cumsum, lengths):
    ts = np.asarray(ts, dtype=np.float32)
    cumsum = np.asarray(cumsum, dtype=np.float32)
    values, indices = C.detect_peaks(torch.from_numpy(ts).cuda(),
                                     torch.from_numpy(cumsum).cuda(), lengths)
    values = values.cpu().numpy()
    indices = indices.cpu().numpy()
    assert values.shape == indices.shape == (1 + len(lengths),)
    series = [ts] + [cumsum[L:] - cumsum[:-L] for L in lengths]
    for j, x in enumerate(series):
        assert x.dtype == np.float32
        assert values[j] == np.max(x), (j, values[j], np.max(x))
        assert indices[j] == np.argmax(x), (j, indices[j], np.argmax(x))


@pytest.mark.parametrize("ts_count", [5, 2048, 70001])
def test_detect_peaks_matches_numpy(C, ts_count):
    lengths = [L for L in LADDER if L < ts_count]
    rng = np.random.default_rng(ts_count)

    ts = rng.normal(0, 1, ts_count).astype(np.float32)
    check_peaks(C, ts, np.cumsum(ts, dtype=np.float32), lengths)

    # all negative: the maximum is negative, not an initial 0
    neg = (-1.0 - np.abs(ts)).astype(np.float32)
    check_peaks(C, neg, np.cumsum(neg, dtype=np.float32), lengths)

    # the same maximum at two indices (and, for the window sums, at every
    # window holding either spike): the lowest index wins
    dup = np.zeros(ts_count, dtype=np.float32)
    dup[[ts_count // 3 + 1, ts_count - 1]] = 7.0
    check_peaks(C, dup, np.cumsum(dup, dtype=np.float32), lengths)

    # no ladder: only the raw peak
    check_peaks(C, ts, np.cumsum(ts, dtype=np.float32), [])


# ---- 4. peaks through the engine ----

def test_engine_trial_peaks_match_numpy(C):
    raw = noise_block(1 << 18, 1)
    eng = make_engine(C, max_dm_trials=len(DMS))
    slot = eng.submit_trials(raw, DMS)
    got = eng.wait_trials(slot)
    plane = eng.dm_time_plane(slot).cpu().numpy()
    for k in range(len(DMS)):
        eng.select_trial(slot, k)
        cumsum = eng.cumsum(slot).cpu().numpy()
        ts = plane[k]
        peaks = got[k]["peaks"]
        assert [p["boxcar_length"] for p in peaks] == [1] + LADDER
        series = [ts] + [cumsum[L:] - cumsum[:-L] for L in LADDER]
        for p, x, thr in zip(peaks, series, got[k]["thresholds"]):
            assert np.float32(p["value"]) == np.max(x)
            assert p["index"] == np.argmax(x)
            snr = np.float32(p["value"]) / (np.float32(thr) / np.float32(6.0))
            assert p["snr"] == pytest.approx(float(snr), rel=1e-6)


# ---- 5. the search finds the true DM ----

@pytest.mark.parametrize("n", [1 << 18, 1 << 20])
def test_dm_trial_search_finds_true_dm(C, n):
    from srtb_amd.pipeline.gpu import DmTrialSearch

    def small_cfg(bits, dm):
        c = Config()
        c.baseband_input_count = n
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

    true_dm = 56.77
    cfg = small_cfg(-16, 0.0)
    t = 0.4 * n / cfg.baseband_sample_rate
    raw8 = synthesize_dispersed_pulse(small_cfg(-8, true_dm), t,
                                      pulse_amp=35.0, noise_sigma=2.0)
    raw = (raw8.view(np.int8).astype(np.int16) * 64).view(np.uint8)
    dms = [0.0, 20.0, 40.0, true_dm, 80.0, 120.0]
    search = DmTrialSearch(cfg, dms, nsamps_reserved=0)
    results = search.search(raw)
    best = search.best(results)
    summary = [(r.dm, round(r.peak_snr, 1), r.peak_boxcar, r.peak_index)
               for r in results]
    print(summary)
    assert [r.dm for r in results] == dms
    assert best.dm == true_dm, summary
    assert best.peak_boxcar == 1, summary
    ts_count = n // 2 // cfg.spectrum_channel_count
    assert abs(best.peak_index - 0.4 * ts_count) <= 2, summary
    runner_up = max(r.peak_snr for r in results if r is not best)
    assert best.peak_snr >= 3.0 * runner_up, summary


# ---- 6. no state leaks and argument checks ----

def test_plain_submit_after_trials_is_unchanged(C):
    raw1, raw2 = noise_block(1 << 18, 2), noise_block(1 << 18, 3)
    fresh = make_engine(C)
    fs = fresh.submit(raw2)
    want = fresh.wait(fs)
    eng = make_engine(C, max_dm_trials=3)
    ts_slot = eng.submit_trials(raw1, [0.0, 25.0, 60.0])
    eng.wait_trials(ts_slot)
    # the other slot, then the slot that just ran the trials
    for expect_slot in (1 - ts_slot, ts_slot):
        slot = eng.submit(raw2)
        assert slot == expect_slot
        res = eng.wait(slot)
        assert res == want
        assert torch.equal(eng.time_series(slot), fresh.time_series(fs))
        assert torch.equal(eng.waterfall(slot), fresh.waterfall(fs))
    with pytest.raises(RuntimeError):
        eng.select_trial(ts_slot, 0)  # the slot holds a plain block again


def test_two_trial_submissions_in_flight(C):
    dms = [25.0, 60.0]
    raws = [noise_block(1 << 18, 10 + i) for i in range(4)]
    eng = make_engine(C, max_dm_trials=len(dms))
    slots = [eng.submit_trials(r, dms) for r in raws[:2]]
    assert slots == [0, 1]
    got = []
    for i, r in enumerate(raws):
        slot = slots[i]
        res = eng.wait_trials(slot)
        got.append((res, eng.dm_time_plane(slot).clone()))
        if i + 2 < len(raws):
            slots.append(eng.submit_trials(raws[i + 2], dms))
    assert slots == [0, 1, 0, 1]
    for r, (res, plane) in zip(raws, got):
        want = yardstick(C, r, dms)
        for k in range(len(dms)):
            assert torch.equal(plane[k], want[k]["ts"])
            assert res[k]["counts"] == want[k]["res"]["counts"]


def test_submit_trials_argument_checks(C):
    raw = noise_block(1 << 18, 4)
    with pytest.raises(RuntimeError, match="max_dm_trials"):
        make_engine(C).submit_trials(raw, [0.0])
    eng = make_engine(C, max_dm_trials=2)
    with pytest.raises(RuntimeError, match="n_trials"):
        eng.submit_trials(raw, [])
    with pytest.raises(RuntimeError, match="n_trials"):
        eng.submit_trials(raw, [0.0, 1.0, 2.0])
    table = make_engine(C, max_dm_trials=2, use_phase_table=True)
    with pytest.raises(RuntimeError, match="use_phase_table"):
        table.submit_trials(raw, [60.0])
    with pytest.raises(RuntimeError, match="max_dm_trials"):
        make_engine(C, max_dm_trials=257)
    # the engine is still usable after the rejections
    slot = eng.submit_trials(raw, [0.0, 60.0])
    assert len(eng.wait_trials(slot)) == 2


# ---- 7. executable ----

@pytest.mark.skipif(not os.path.exists(BIN), reason="native binaries not built")
def test_srtb_backend_dm_trial_list(tmp_path):
    """One noise block, then one pulse block at DM 60, searched from dm 0
    with a six-trial list."""
    import glob

    cfg = Config()
    cfg.baseband_input_count = n = 1 << 18
    cfg.spectrum_channel_count = 1 << 6
    cfg.baseband_input_bits = -8
    cfg.baseband_freq_low = 1400.0
    cfg.baseband_bandwidth = 64.0
    cfg.baseband_sample_rate = 128e6
    cfg.dm = 60.0
    rng = np.random.default_rng(0)
    noise = np.clip(np.round(rng.normal(0, 2, n)), -128,
                    127).astype(np.int8).view(np.uint8)
    pulse = synthesize_dispersed_pulse(cfg, 0.4 * n / cfg.baseband_sample_rate,
                                       pulse_amp=40.0, noise_sigma=2.0)
    rec = tmp_path / "rec.bin"
    np.concatenate([noise, pulse]).tofile(rec)

    out = subprocess.run(
        [BIN, "--input_file_path", str(rec),
         "--baseband_input_count", str(n), "--baseband_input_bits", "-8",
         "--spectrum_channel_count", str(cfg.spectrum_channel_count),
         "--baseband_freq_low", "1400", "--baseband_bandwidth", "64",
         "--baseband_sample_rate", "128e6", "--dm", "0",
         "--dm_trial_list", "0,20,40,60,80,120",
         "--baseband_reserve_sample", "0",
         "--mitigate_rfi_average_method_threshold", "1e30",
         "--mitigate_rfi_spectral_kurtosis_threshold", "1e30",
         "--signal_detect_signal_noise_threshold", "6",
         "--signal_detect_max_boxcar_length", "16",
         "--baseband_output_file_prefix", str(tmp_path) + "/out_"],
        capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr
    assert "blocks=2 detections=1" in out.stdout, (out.stdout, out.stderr)
    assert (out.stdout + out.stderr).count("dm-trials block") == 2

    dmts = glob.glob(str(tmp_path / "out_*.dmt"))
    assert len(dmts) == 1, dmts
    rows = np.loadtxt(dmts[0])
    assert rows.shape == (6, 6), rows
    assert list(rows[:, 0]) == [0, 20, 40, 60, 80, 120]
    assert rows[np.argmax(rows[:, 1]), 0] == 60.0, rows

    npys = glob.glob(str(tmp_path / "out_*.npy"))
    assert len(npys) == 1
    ts_count = n // 2 // cfg.spectrum_channel_count
    assert np.load(npys[0]).shape == (cfg.spectrum_channel_count, ts_count)
    stem = dmts[0][:-len(".dmt")]
    tim = np.fromfile(stem + ".1.tim", dtype=np.float32)
    assert tim.size == ts_count
    assert abs(int(np.argmax(tim)) - 819) <= 2
    # the dumped series is the best trial's: its peak is the sidecar's
    best = rows[np.argmax(rows[:, 1])]
    assert int(best[3]) == int(np.argmax(tim)) or int(best[2]) != 1
