"""Filterbank output without a GPU: the NumPy oracle, the overlap rounding,
the .fil writer and reader, srtb_amd.main end to end on the CPU pipelines and
the configuration keys of both apps."""

import os
import subprocess

import numpy as np
import pytest

from srtb_amd import ref
from srtb_amd.config import Config, parse_args, parse_config_file
from srtb_amd.io.writers import (FilterbankWriter, filterbank_header,
                                 read_filterbank)
from srtb_amd.pipeline.cpu import synthesize_dispersed_pulse

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "bin", "srtb-backend")


# ---- 1. oracle geometry ----

def hand_waterfall():
    """[8][16], every |wf|^2 distinct: power of (row, t) = 1 + 16 row + t,
    row 5 zapped."""
    p = 1.0 + 16.0 * np.arange(8)[:, None] + np.arange(16)[None, :]
    wf = (np.sqrt(p) * np.exp(1j * 0.7 * np.arange(16))[None, :])
    wf[5] = 0
    p[5] = 0
    return wf.astype(np.complex128), p


@pytest.mark.parametrize("reverse", [False, True])
def test_oracle_no_scrunch_is_the_transposed_power(reverse):
    wf, p = hand_waterfall()
    P = ref.filterbank_block(wf, 16, 1, 1, reverse)
    assert P.shape == (16, 8) and P.dtype == np.float64
    want = p[::-1].T if reverse else p.T
    np.testing.assert_allclose(P, want, rtol=1e-12)
    assert (P[:, 2 if reverse else 5] == 0).all()


@pytest.mark.parametrize("reverse", [False, True])
@pytest.mark.parametrize("tscrunch,fscrunch,valid",
                         [(4, 1, 16), (1, 2, 16), (2, 4, 12), (4, 8, 14)])
def test_oracle_scrunch_cells(reverse, tscrunch, fscrunch, valid):
    wf, p = hand_waterfall()
    P = ref.filterbank_block(wf, valid, tscrunch, fscrunch, reverse)
    R, C = valid // tscrunch, 8 // fscrunch
    assert P.shape == (R, C)
    for r in range(R):
        for c in range(C):
            lo = 8 - (c + 1) * fscrunch if reverse else c * fscrunch
            cell = p[lo:lo + fscrunch, r * tscrunch:(r + 1) * tscrunch]
            assert P[r, c] == pytest.approx(cell.sum(), rel=1e-12), (r, c)


def test_oracle_rejects_bad_geometry():
    wf, _ = hand_waterfall()
    with pytest.raises(ValueError):
        ref.filterbank_block(wf, 16, 1, 3, False)
    with pytest.raises(ValueError):
        ref.filterbank_block(wf, 17, 1, 1, False)


def test_oracle_quantize():
    P = np.array([[10.0, 5.0, 0.0], [12.0, 5.0, 0.0], [8.0, 5.0, 0.0],
                  [1000.0, 5.0, 0.0], [-1000.0, 5.0, 0.0]])
    mean = np.array([10.0, 5.0, 0.0])
    std = np.array([2.0, 0.0, 0.0])
    q = ref.filterbank_quantize(P, mean, std)
    assert q.dtype == np.uint8
    assert q[:, 0].tolist() == [64, 80, 48, 255, 0]
    assert (q[:, 1:] == ref.FILTERBANK_QUANT_LEVEL).all()
    assert ref.FILTERBANK_QUANT_LEVEL == 64
    assert ref.FILTERBANK_QUANT_PER_SIGMA == 16


# ---- 2. overlap rounding ----

@pytest.mark.parametrize("t", [1, 2, 16, 64])
@pytest.mark.parametrize("dm", [0.0, -5.0, -56.77, -478.8])
def test_nsamps_reserved_time_multiple(t, dm):
    n, s = 1 << 26, 1 << 8
    args = (n, s, 1405.0 + 32.0, -64.0, 128e6, dm, True)
    old = ref.nsamps_reserved(*args)
    got = ref.nsamps_reserved(*args, time_multiple=t)
    assert (n - got) % (2 * s * t) == 0
    assert got >= old
    if t == 1:
        assert got == old
    if dm != 0.0:
        assert 0 < got < n
    assert got - old < 2 * s * t


def test_valid_rows_differ_from_ts_count():
    n, s = 1 << 20, 1 << 6
    res = 2 * s * 16 * 3
    v = ref.filterbank_valid_rows(n, s, res)
    assert v == (n - res) // (2 * s)
    ts_count = n // 2 // s - res // s
    assert v - ts_count == res // (2 * s)


# ---- 3. writer and reader ----

@pytest.mark.parametrize("nbits", [8, 32])
def test_writer_reader_round_trip(tmp_path, nbits):
    kw = ref.filterbank_header_fields(1400.0, 64.0, 128e6, 64, 4, 2)
    assert kw["nchans"] == 32
    assert kw["foff"] == -2.0
    assert kw["fch1"] == 1464.0 - 1.0
    assert kw["tsamp"] == 2 * 64 * 4 / 128e6
    kw.update(nbits=nbits, tstart=60000.5)
    rng = np.random.default_rng(nbits)
    R, C = 7, 32
    if nbits == 8:
        blocks = [rng.integers(0, 256, (R, C), dtype=np.uint8)
                  for _ in range(2)]
    else:
        blocks = [rng.normal(size=(R, C)).astype(np.float32)
                  for _ in range(2)]
    path = tmp_path / "x.fil"
    with FilterbankWriter(str(path), kw) as w:
        for b in blocks:
            w.append(b)
        assert w.rows == 2 * R
        with pytest.raises(ValueError):
            w.append(blocks[0][:, :5])
        with pytest.raises(ValueError):
            w.append(blocks[0].astype(np.float64))
    header, data = read_filterbank(str(path))
    assert header["header_len"] == len(filterbank_header(**kw))
    assert os.path.getsize(path) == header["header_len"] + 2 * R * C * nbits // 8
    for key in ("fch1", "foff", "tsamp", "nchans", "nbits", "tstart"):
        assert header[key] == kw[key], key
    assert header["source_name"] == "srtb"
    assert data.shape == (2 * R, C)
    assert data.dtype == (np.uint8 if nbits == 8 else np.float32)
    assert np.array_equal(data, np.concatenate(blocks))


def test_header_fields_negative_bandwidth():
    kw = ref.filterbank_header_fields(1437.0, -64.0, 128e6, 2048, 16, 1)
    assert kw["foff"] == -64.0 / 2048
    assert kw["fch1"] == 1437.0 - 64.0 / 4096
    assert kw["nchans"] == 2048


# ---- 4. end to end through srtb_amd.main on the CPU pipelines ----

N, S, TSCRUNCH = 1 << 18, 1 << 6, 4


def pulse_cfg():
    cfg = Config()
    cfg.baseband_input_count = N
    cfg.spectrum_channel_count = S
    cfg.baseband_input_bits = -8
    cfg.baseband_freq_low = 1400.0
    cfg.baseband_bandwidth = 64.0
    cfg.baseband_sample_rate = 128e6
    cfg.dm = 60.0
    return cfg


PULSE_INDEX = int(0.4 * N)  # sample of the pulse within the second block


def pulse_recording(path):
    """noise, pulse, noise: three blocks of int8 baseband.  width=1 makes the
    pulse fill the band (the default click only reaches the lowest few MHz)."""
    cfg = pulse_cfg()
    rng = np.random.default_rng(0)
    noise = [np.clip(np.round(rng.normal(0, 2, N)), -128,
                     127).astype(np.int8).view(np.uint8) for _ in range(2)]
    pulse = synthesize_dispersed_pulse(
        cfg, PULSE_INDEX / cfg.baseband_sample_rate, pulse_amp=40.0,
        noise_sigma=2.0, width=1)
    np.concatenate([noise[0], pulse, noise[1]]).tofile(path)


APP_ARGS = [
    "--baseband_input_count", str(N), "--baseband_input_bits", "-8",
    "--spectrum_channel_count", str(S), "--baseband_freq_low", "1400",
    "--baseband_bandwidth", "64", "--baseband_sample_rate", "128e6",
    "--dm", "60", "--mitigate_rfi_average_method_threshold", "1e30",
    "--mitigate_rfi_spectral_kurtosis_threshold", "1e30",
    # zeroes the whole spectrum of channels 10 and 11
    "--mitigate_rfi_freq_list", "1410-1412",
    "--signal_detect_signal_noise_threshold", "6",
    "--signal_detect_max_boxcar_length", "16",
    "--filterbank_tscrunch", str(TSCRUNCH),
]


def check_pulse_file(path, nbits):
    """3R rows; the pulse sits in the row its absolute sample falls into and
    is bright there across the band."""
    header, data = read_filterbank(str(path))
    R, C = N // (2 * S * TSCRUNCH), S
    assert header["nbits"] == nbits and header["nchans"] == C
    assert header["tsamp"] == 2 * S * TSCRUNCH / 128e6
    assert header["foff"] == -1.0 and header["fch1"] == 1463.5
    assert data.shape == (3 * R, C)
    x = data.astype(np.float64)
    zapped = (x == x[0:1]).all(axis=0)
    # descending frequency: 1410-1412 MHz are output channels 52 and 53
    assert zapped[[52, 53]].all() and zapped.sum() <= 4, np.nonzero(zapped)
    live = x[:, ~zapped]
    row = int(np.argmax(live.sum(axis=1)))
    want = (N + PULSE_INDEX) // (2 * S * TSCRUNCH)
    assert abs(row - want) <= 1, (row, want)
    med = np.median(live, axis=0)
    mad = 1.4826 * np.median(np.abs(live - med), axis=0)
    bright = live[row] > med + 6 * mad
    assert bright.sum() >= 0.75 * live.shape[1], bright.sum()
    return row


def test_main_cpu_end_to_end_float(tmp_path):
    from srtb_amd.main import main
    rec = tmp_path / "rec.bin"
    pulse_recording(rec)
    out = tmp_path / "out.fil"
    rc = main(APP_ARGS + [
        "--device", "cpu", "--input_file_path", str(rec),
        "--filterbank_output_path", str(out), "--filterbank_nbits", "32",
        "--baseband_output_file_prefix", str(tmp_path) + "/p_"])
    assert rc == 0
    check_pulse_file(out, 32)


def test_main_cpu_end_to_end_8bit(tmp_path):
    from srtb_amd.main import main
    rec = tmp_path / "rec.bin"
    pulse_recording(rec)
    out = tmp_path / "out.fil"
    rc = main(APP_ARGS + [
        "--device", "cpu", "--input_file_path", str(rec),
        "--filterbank_output_path", str(out), "--filterbank_nbits", "8",
        "--baseband_output_file_prefix", str(tmp_path) + "/p_"])
    assert rc == 0
    row = check_pulse_file(out, 8)
    _, data = read_filterbank(str(out))
    assert data.dtype == np.uint8
    # per-block normalisation: every live channel of every block sits at 64
    R = N // (2 * S * TSCRUNCH)
    live = np.delete(data, [52, 53], axis=1)
    for b in range(3):
        m = live[b * R:(b + 1) * R].mean(axis=0)
        assert np.abs(m - 64).max() < 1.5, (b, m)
    assert (data[:, [52, 53]] == 64).all()
    assert data[row].max() == 255


TWO_POL_ARGS = [
    "--baseband_format_type", "naocpsr_snap1",
    "--baseband_input_count", str(1 << 16), "--spectrum_channel_count", "64",
    "--baseband_input_bits", "-8", "--baseband_freq_low", "1400",
    "--baseband_bandwidth", "64", "--baseband_sample_rate", "128e6",
    "--dm", "40", "--baseband_reserve_sample", "0",
    "--mitigate_rfi_average_method_threshold", "1e30",
    "--mitigate_rfi_spectral_kurtosis_threshold", "1e30",
    "--signal_detect_signal_noise_threshold", "6",
    "--signal_detect_max_boxcar_length", "16",
    "--filterbank_tscrunch", "4", "--filterbank_nbits", "32",
]


def check_two_pol_files(tmp_path):
    """one file per data stream, the pulse of block 1 in both."""
    R = (1 << 16) // (2 * 64 * 4)
    planes = []
    for k in range(2):
        header, data = read_filterbank(str(tmp_path / f"pol_s{k}.fil"))
        assert data.shape == (2 * R, 64) and header["nbits"] == 32
        row = int(np.argmax(data.astype(np.float64).sum(axis=1)))
        want = ((1 << 16) + (1 << 15)) // (2 * 64 * 4)
        assert abs(row - want) <= 1, (k, row, want)
        planes.append(data)
    assert not np.array_equal(planes[0], planes[1])
    assert not os.path.exists(tmp_path / "pol.fil")
    return planes


def test_main_cpu_two_pol_writes_one_file_per_stream(tmp_path):
    from srtb_amd.main import main
    from tests.test_main_app import make_2pol_recording
    _, rec = make_2pol_recording(tmp_path)
    rc = main(TWO_POL_ARGS + [
        "--device", "cpu", "--input_file_path", rec,
        "--filterbank_output_path", str(tmp_path / "pol.fil"),
        "--baseband_output_file_prefix", str(tmp_path) + "/p2_"])
    assert rc == 0
    check_two_pol_files(tmp_path)


def test_main_rejects_trials_with_filterbank(tmp_path):
    from srtb_amd.main import main
    rec = tmp_path / "rec.bin"
    np.zeros(N, dtype=np.uint8).tofile(rec)
    with pytest.raises(SystemExit, match="dm_trial_list"):
        main(APP_ARGS + ["--device", "cpu", "--input_file_path", str(rec),
                         "--filterbank_output_path", str(tmp_path / "o.fil"),
                         "--dm_trial_list", "0, 60"])
    with pytest.raises(SystemExit, match="filterbank_tscrunch"):
        main(APP_ARGS + ["--device", "cpu", "--input_file_path", str(rec),
                         "--filterbank_output_path", str(tmp_path / "o.fil"),
                         "--filterbank_tscrunch", "12"])


def test_filterbank_paths():
    from srtb_amd.main import filterbank_paths
    cfg = Config()
    cfg.filterbank_output_path = "/data/run.1/obs.fil"
    assert filterbank_paths(cfg, 1, 0, 1) == ["/data/run.1/obs.fil"]
    assert filterbank_paths(cfg, 2, 0, 1) == ["/data/run.1/obs_s0.fil",
                                              "/data/run.1/obs_s1.fil"]
    assert filterbank_paths(cfg, 2, 3, 8) == ["/data/run.1/obs_s0_r3.fil",
                                              "/data/run.1/obs_s1_r3.fil"]
    cfg.filterbank_output_path = "/data/run.1/obs"
    assert filterbank_paths(cfg, 1, 1, 2) == ["/data/run.1/obs_r1"]


# ---- 5. configuration twins ----

def test_python_config_keys(tmp_path):
    cfg = Config()
    assert cfg.filterbank_output_path == ""
    assert (cfg.filterbank_tscrunch, cfg.filterbank_fscrunch,
            cfg.filterbank_nbits, cfg.filterbank_tstart_mjd) == (16, 1, 8, 0.0)
    path = tmp_path / "c.cfg"
    path.write_text("filterbank_output_path = /tmp/a.fil  # out\n"
                    "filterbank_tscrunch = 2 ** 5\n"
                    "filterbank_tstart_mjd = 60000 + 0.25\n")
    cfg = parse_config_file(str(path))
    assert cfg.filterbank_output_path == "/tmp/a.fil"
    assert cfg.filterbank_tscrunch == 32
    assert cfg.filterbank_tstart_mjd == 60000.25
    cfg = parse_args(["--config_file_name", str(path),
                      "--filterbank_fscrunch", "4", "--filterbank_nbits=32"])
    assert (cfg.filterbank_tscrunch, cfg.filterbank_fscrunch,
            cfg.filterbank_nbits) == (32, 4, 32)


def dry_run(*args):
    return subprocess.run([BIN, "--dry-run", *args], capture_output=True,
                          text=True, timeout=60)


def keyed(stdout):
    return dict(line.split(" = ", 1) for line in stdout.splitlines()
                if " = " in line)


needs_bin = pytest.mark.skipif(not os.path.exists(BIN),
                               reason="native binaries not built")


@needs_bin
def test_native_dry_run_is_silent_by_default():
    out = dry_run()
    assert out.returncode == 0, out.stderr
    assert "filterbank" not in out.stdout


@needs_bin
def test_native_dry_run_echoes_keys():
    out = dry_run("--filterbank_output_path", "/tmp/a.fil",
                  "--filterbank_tscrunch", "2**5", "--filterbank_fscrunch",
                  "4", "--filterbank_nbits", "32", "--filterbank_tstart_mjd",
                  "60000 + 0.25")
    assert out.returncode == 0, out.stderr
    k = keyed(out.stdout)
    assert k["filterbank_output_path"] == "/tmp/a.fil"
    assert int(k["filterbank_tscrunch"]) == 32
    assert int(k["filterbank_fscrunch"]) == 4
    assert int(k["filterbank_nbits"]) == 32
    assert float(k["filterbank_tstart_mjd"]) == 60000.25
    out = dry_run("--filterbank_output_path", "/tmp/a.fil")
    k = keyed(out.stdout)
    assert (int(k["filterbank_tscrunch"]), int(k["filterbank_fscrunch"]),
            int(k["filterbank_nbits"])) == (16, 1, 8)


@needs_bin
def test_native_overlap_rule_matches_python():
    """With the path set the overlap leaves whole output rows, and equals
    Python's."""
    n, s, t = 1 << 24, 1 << 8, 16
    args = ["--baseband_input_count", str(n), "--spectrum_channel_count",
            str(s), "--baseband_freq_low", "1437", "--baseband_bandwidth",
            "-64", "--baseband_sample_rate", "128e6", "--dm", "-56.77",
            "--input_file_path", "/nonexistent"]
    off = int(keyed(dry_run(*args).stdout)["nsamps_reserved"])
    on = int(keyed(dry_run(*args, "--filterbank_output_path", "/tmp/a.fil",
                           "--filterbank_tscrunch", str(t)
                           ).stdout)["nsamps_reserved"])
    want_off = ref.nsamps_reserved(n, s, 1437.0, -64.0, 128e6, -56.77)
    want_on = ref.nsamps_reserved(n, s, 1437.0, -64.0, 128e6, -56.77,
                                  time_multiple=t)
    assert (off, on) == (want_off, want_on)
    assert (n - on) % (2 * s * t) == 0


@needs_bin
def test_native_rejects_trials_with_filterbank():
    out = dry_run("--filterbank_output_path", "/tmp/a.fil",
                  "--dm_trial_list", "0, 60")
    assert out.returncode != 0
    assert "dm_trial_list" in out.stderr + out.stdout
    out = dry_run("--filterbank_output_path", "/tmp/a.fil",
                  "--filterbank_tscrunch", "12")
    assert out.returncode != 0
    assert "filterbank_tscrunch" in out.stderr + out.stdout
