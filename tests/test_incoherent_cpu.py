"""CPU tests of the incoherent DM-offset search: the delay table, the oracle
functions, the streaming CpuIncoherentSearch and the application wiring."""

import numpy as np
import pytest

from srtb_amd import ref
from srtb_amd.config import Config, parse_args
from srtb_amd.pipeline.cpu import synthesize_dispersed_pulse


# ---- delay table ----

def test_delay_table_hand_computed():
    # f = 1400, 1300, 1200, 1100 MHz; f^-2 in 1e-7 MHz^-2:
    #   5.1020408, 5.9171598, 6.9444444, 8.2644628
    # D * 10 / tsamp = 4.148808e3 * 10 / 1e-3 = 4.148808e7, so
    #   delta = +10: 4.148808 * (0, 0.8151190, 1.8424036, 3.1624220)
    #              = 0, 3.3818, 7.6438, 13.1203         -> 0, 3, 8, 13
    #   delta = -10: 4.148808 * (3.1624220, 2.3473030, 1.3200184, 0)
    #              = 13.1203, 9.7385, 5.4765, 0         -> 13, 10, 5, 0
    d = ref.incoherent_delays(1400.0, -100.0, 4, 1e-3, [10.0, -10.0, 0.0])
    assert d.dtype == np.int32 and d.shape == (3, 4)
    assert d.tolist() == [[0, 3, 8, 13], [13, 10, 5, 0], [0, 0, 0, 0]]


def test_delay_table_is_monotone_and_rounds_ties_to_even():
    offsets = [-3.0, -0.25, 0.0, 0.5, 7.0]
    d = ref.incoherent_delays(1463.5, -1.0, 64, 16e-6, offsets)
    assert (d >= 0).all()
    for row, delta in zip(d, offsets):
        step = np.diff(row.astype(np.int64))
        assert (step >= 0).all() if delta >= 0 else (step <= 0).all()
    assert (d[2] == 0).all()
    assert d[4].max() == d.max() > d[3].max() > 0
    # np.rint: 0.5 -> 0, 1.5 -> 2, 2.5 -> 2
    assert np.rint([0.5, 1.5, 2.5]).tolist() == [0.0, 2.0, 2.0]


def test_delay_table_rejections():
    with pytest.raises(ValueError):
        ref.incoherent_delays(1400.0, -100.0, 4, 0.0, [1.0])
    with pytest.raises(ValueError):
        ref.incoherent_delays(1400.0, -100.0, 4, 1e-3, [float("nan")])
    with pytest.raises(ValueError):  # a channel at or below 0 MHz
        ref.incoherent_delays(300.0, -100.0, 4, 1e-3, [1.0])
    with pytest.raises(ValueError):  # ascending frequency: negative delays
        ref.incoherent_delays(1100.0, 100.0, 4, 1e-3, [10.0])
    with pytest.raises(ValueError):  # beyond 2^20 rows
        ref.incoherent_delays(1400.0, -100.0, 4, 1e-9, [10.0])


# ---- dedisperse / detect oracles ----

def test_dedisperse_by_hand():
    window = np.arange(15, dtype=np.float64).reshape(5, 3)  # D = 2, R = 3
    delays = np.array([[0, 0, 0], [2, 0, 1]], dtype=np.int32)
    Y = ref.incoherent_dedisperse(window, delays, 3)
    assert Y[0].tolist() == [0 + 1 + 2, 3 + 4 + 5, 6 + 7 + 8]
    assert Y[1].tolist() == [6 + 1 + 5, 9 + 4 + 8, 12 + 7 + 11]
    with pytest.raises(ValueError):
        ref.incoherent_dedisperse(window, delays + 1, 3)


def test_detect_by_hand():
    Y = np.array([[0, 0, 0, 8, 0, 0, 0, 0]], dtype=np.float64)
    det = ref.incoherent_detect(Y, 1.5, 16)
    assert det["lengths"] == [1, 2, 4, 8, 16]
    assert det["mu"][0] == 1.0
    # z = -1 except z[3] = 7; length 1: peak 7 at 3, rms = sqrt(56 / 8)
    assert det["peak"][0, 0] == 7.0 and det["index"][0, 0] == 3
    assert det["rms"][0, 0] == np.sqrt(7.0) and det["count"][0, 0] == 1
    assert det["snr"][0, 0] == 7.0 / np.sqrt(7.0)
    # length 2: b[i] = z[i+1] + z[i+2], i < 6: 6 at i = 1 and 2 -> index 1
    assert det["peak"][0, 1] == 6.0 and det["index"][0, 1] == 1
    assert det["count"][0, 1] == 2
    # lengths 8 and 16 have no window
    assert np.isneginf(det["peak"][0, 3:]).all()
    assert (det["index"][0, 3:] == -1).all() and (det["snr"][0, 3:] == 0).all()


# ---- streaming ----

@pytest.mark.parametrize("tsamp,deep", [(1e-3, False), (2.5e-4, True)])
def test_streaming_equals_the_whole_array(tsamp, deep):
    R, C, offsets = 8, 16, [-30.0, 0.0, 12.5, 40.0]
    s = ref.CpuIncoherentSearch(R, C, 1463.5, -4.0, tsamp, offsets, 2.0, 4)
    assert (s.d_max > 2 * R) == deep and s.d_max > 0
    rng = np.random.default_rng(5)
    planes = [rng.integers(0, 16, (R, C)).astype(np.float64) for _ in range(5)]
    # the stream with D_max rows of zeros before it: global row g is row
    # g + D_max, and block b's window starts at row b * R
    stream = np.concatenate([np.zeros((s.d_max, C))] + planes)
    whole = ref.incoherent_dedisperse(stream, s.delays, 5 * R)
    for b, plane in enumerate(planes):
        res = s.add(plane)
        assert res["block"] == b
        assert res["first_row"] == b * R - s.d_max
        assert res["valid"] == (b * R >= s.d_max)
        assert bool(res["trials"]) == res["valid"]
        assert np.array_equal(res["Y"], whole[:, b * R:(b + 1) * R])
    s.reset()
    res = s.add(planes[4])
    assert res["block"] == 0 and res["first_row"] == -s.d_max
    assert np.array_equal(
        res["Y"], ref.incoherent_dedisperse(
            np.concatenate([np.zeros((s.d_max, C)), planes[4]]), s.delays, R))


def test_constructor_limits():
    ok = dict(R=8, C=16, fch1=1463.5, foff=-4.0, tsamp=1e-3, offsets=[1.0],
              snr_threshold=6.0, max_boxcar=4)
    ref.CpuIncoherentSearch(**ok)
    for kw in (dict(offsets=[]), dict(offsets=[0.0] * 1025), dict(R=1),
               dict(R=16385), dict(max_boxcar=0), dict(offsets=[1e9]),
               dict(offsets=[2e6], C=2048, foff=-0.03)):
        with pytest.raises(ValueError):
            ref.CpuIncoherentSearch(**{**ok, **kw})


# ---- recovery of a swept impulse ----

def test_a_swept_impulse_is_recovered_at_its_offset():
    R, C, tsamp = 64, 32, 2.5e-5
    fch1, foff = 1499.0, -2.0
    offsets = [-4.0, -2.0, 0.0, 2.0, 4.0, 6.0]
    true = 4.0
    s = ref.CpuIncoherentSearch(R, C, fch1, foff, tsamp, offsets, 5.0, 8)
    sweep = ref.incoherent_delays(fch1, foff, C, tsamp, [true])[0]
    assert sweep.max() > 8  # the other trials smear it over many rows
    rng = np.random.default_rng(6)
    blocks = 4
    stream = rng.normal(0.0, 1.0, (blocks * R, C))
    g0 = 2 * R + 11  # the impulse's row at the top channel
    stream[g0 + sweep, np.arange(C)] += 12.0
    best = None
    for b in range(blocks):
        res = s.add(stream[b * R:(b + 1) * R])
        for tr in res["trials"]:
            for ln in tr["lengths"]:
                cand = (ln["snr"], tr["offset"], ln["boxcar_length"],
                        res["first_row"] + ln["index"])
                if best is None or cand > best:
                    best = cand
    snr, offset, length, row = best
    assert offset == true and length == 1 and row == g0
    # the rms includes the impulse: one row of R cannot exceed sqrt(R - 1),
    # and 32 channels * 12 against a noise rms of sqrt(32) comes close to it
    assert 0.95 * np.sqrt(R - 1) < snr < np.sqrt(R - 1)


# ---- applications ----

def test_config_keys_parse():
    cfg = parse_args(["--incoherent_dm_offsets", "-1, 0, 0.5, 2 - 1/2",
                      "--incoherent_output_path", "/tmp/x.cand"])
    assert cfg.incoherent_offsets() == [-1.0, 0.0, 0.5, 1.5]
    assert cfg.incoherent_output_path == "/tmp/x.cand"
    assert Config().incoherent_offsets() == []
    with pytest.raises(Exception):
        parse_args(["--incoherent_dm_offsets", "1,,2"])


N, S, TSCRUNCH = 1 << 18, 1 << 6, 16
PULSE_INDEX = int(0.4 * N)

APP_ARGS = [
    "--baseband_input_count", str(N), "--baseband_input_bits", "-8",
    "--spectrum_channel_count", str(S), "--baseband_freq_low", "1400",
    "--baseband_bandwidth", "64", "--baseband_sample_rate", "128e6",
    "--dm", "60", "--mitigate_rfi_average_method_threshold", "1e30",
    "--mitigate_rfi_spectral_kurtosis_threshold", "1e30",
    "--signal_detect_signal_noise_threshold", "6",
    "--signal_detect_max_boxcar_length", "16",
    "--filterbank_tscrunch", str(TSCRUNCH),
]


def offset_pulse_recording(path, dm=62.0):
    """noise, a pulse at `dm` (the run dedisperses at 60), noise."""
    cfg = Config()
    cfg.baseband_input_count = N
    cfg.spectrum_channel_count = S
    cfg.baseband_input_bits = -8
    cfg.baseband_freq_low = 1400.0
    cfg.baseband_bandwidth = 64.0
    cfg.baseband_sample_rate = 128e6
    cfg.dm = dm
    rng = np.random.default_rng(0)
    noise = [np.clip(np.round(rng.normal(0, 2, N)), -128,
                     127).astype(np.int8).view(np.uint8) for _ in range(2)]
    pulse = synthesize_dispersed_pulse(cfg, PULSE_INDEX / 128e6,
                                       pulse_amp=40.0, noise_sigma=2.0,
                                       width=1)
    np.concatenate([noise[0], pulse, noise[1]]).tofile(path)


def read_candidates(path):
    """[(block, time, dm, boxcar, snr)]"""
    out = []
    for line in open(path):
        b, t, dm, l, snr = line.split()
        out.append((int(b), float(t), float(dm), int(l), float(snr)))
    return out


def check_candidates(path):
    cands = read_candidates(path)
    assert cands
    best = max(cands, key=lambda c: c[4])
    assert best[2] == 62.0, best
    tsamp = 2 * S * TSCRUNCH / 128e6
    assert abs(best[1] - (N + PULSE_INDEX) / 128e6) <= (best[3] + 1) * tsamp
    zero = [c[4] for c in cands if c[2] == 60.0 and c[0] == best[0]]
    assert not zero or max(zero) < best[4]
    return cands


def test_main_cpu_writes_the_injected_offset(tmp_path):
    from srtb_amd.main import main
    rec = tmp_path / "rec.bin"
    offset_pulse_recording(rec)
    out = tmp_path / "out.cand"
    rc = main(APP_ARGS + [
        "--device", "cpu", "--input_file_path", str(rec),
        "--incoherent_dm_offsets", "-2,-1,0,1,2,3,4",
        "--incoherent_output_path", str(out),
        "--baseband_output_file_prefix", f"{tmp_path}/o_"])
    assert rc == 0
    check_candidates(out)
    assert not list(tmp_path.glob("*.fil"))  # the plane alone, no file


@pytest.mark.parametrize("extra,match", [
    (["--dm_trial_list", "59,60,61"], "dm_trial_list"),
    (["--filterbank_polarization", "I", "--filterbank_output_path", "x.fil",
      "--baseband_format_type", "naocpsr_snap1"], "filterbank_polarization"),
])
def test_main_mutual_exclusions(tmp_path, extra, match):
    from srtb_amd.main import main
    with pytest.raises(SystemExit, match=match):
        main(APP_ARGS + ["--device", "cpu", "--input_file_path", "none.bin",
                         "--incoherent_dm_offsets", "0,1",
                         "--incoherent_output_path", str(tmp_path / "c.cand")]
             + extra)


def test_main_needs_both_keys(tmp_path):
    from srtb_amd.main import main
    base = APP_ARGS + ["--device", "cpu", "--input_file_path", "none.bin"]
    with pytest.raises(SystemExit, match="incoherent_output_path"):
        main(base + ["--incoherent_dm_offsets", "0,1"])
    with pytest.raises(SystemExit, match="incoherent_dm_offsets"):
        main(base + ["--incoherent_output_path", str(tmp_path / "c.cand")])


def test_candidate_lines_format():
    res = {"valid": True, "first_row": 100, "block": 3, "trials": [
        {"offset": 0.5, "mean": 0.0, "lengths": [
            {"boxcar_length": 1, "peak": 9.0, "index": 7, "rms": 1.5,
             "count": 2, "snr": 6.0},
            {"boxcar_length": 2, "peak": 1.0, "index": 0, "rms": 1.0,
             "count": 0, "snr": 1.0}]}]}
    assert ref.incoherent_candidate_lines(res, 16e-6, 60.0) == [
        "3 0.001712000 60.500000 1 6.000000\n"]
    res["valid"] = False
    assert ref.incoherent_candidate_lines(res, 16e-6, 60.0) == []
