"""CPU tests of pulsar folding: the phase words in fixed point, the oracle
fold, config parsing in Python and in the native dry-run, and
``srtb_amd.main --device cpu`` end to end on synthetic pulse trains."""

import math
import os
import subprocess
from fractions import Fraction

import numpy as np
import pytest

from srtb_amd import ref
from srtb_amd.config import Config, parse_args, parse_config_file
from srtb_amd.io.writers import fold_subint_paths, read_fold_meta

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "bin", "srtb-backend")

T = 1 << 64
N, S = 1 << 18, 1 << 6
RATE = 128e6


# ---- phase words ----

def exact_words(n0, S_, rate, f0, phase0):
    """f1 = 0 in exact rational arithmetic on the rounded step."""
    step = round(Fraction(f0) / Fraction(rate) * T)
    p0 = Fraction(phase0) - math.floor(Fraction(phase0))
    return (int(p0 * T) + n0 * step) % T, (2 * S_ * step) % T


@pytest.mark.parametrize("n0", [0, 1, 12345, (1 << 28) + 7, 10 ** 12 + 1,
                                1 << 44])
@pytest.mark.parametrize("f0,phase0", [(1 / 0.455, 0.0), (2713.7, 0.3),
                                       (641.9282, -0.25), (29.946923, 7.875)])
def test_phase_words_exact_without_f1(n0, f0, phase0):
    got = ref.fold_phase_words(n0, N, 0, S, RATE, f0, 0.0, phase0)
    assert got == exact_words(n0, S, RATE, f0, phase0)
    # the overlap moves nothing while f1 = 0
    assert got == ref.fold_phase_words(n0, N, 2 * S * 5, S, RATE, f0, 0.0,
                                       phase0)


def test_phase_step_is_the_rounded_ratio():
    assert ref.fold_phase_step(128e6, 1e6) == T // 128
    assert ref.fold_phase_step(RATE, 2713.7) == round(
        Fraction(2713.7) / Fraction(RATE) * T)


@pytest.mark.parametrize("f1", [1e-9, -1e-9, 3.7e-13, -1e-15])
@pytest.mark.parametrize("t", [0.0, 0.5, 77.7, 1000.0])
def test_phase_words_with_f1(f1, t):
    f0, phase0, reserved = 2713.7, 0.3, 2 * S * 5
    n0 = int(t * RATE)
    phi, dphi = ref.fold_phase_words(n0, N, reserved, S, RATE, f0, f1, phase0)
    phi0, dphi0 = exact_words(n0, S, RATE, f0, phase0)
    t0 = Fraction(n0) / Fraction(RATE)
    t_mid = Fraction(n0 + (N - reserved) // 2) / Fraction(RATE)
    q = Fraction(f1) * t0 * t0 / 2
    want_phi = (phi0 + round((q - math.floor(q)) * T)) % T
    want_dphi = (dphi0 + round(Fraction(f1) * t_mid * 2 * S / Fraction(RATE)
                               * T)) % T

    def dist(a, b):
        d = (a - b) % T
        return min(d, T - d)

    assert dist(phi, want_phi) <= 1 << 34   # 2^-30 turn
    assert dist(dphi, want_dphi) <= 1 << 34


def test_fold_check_rejections():
    ref.fold_check(S, RATE, 2713.7, 64)
    for nbin in (0, 1, 65537):
        with pytest.raises(ValueError, match="fold_nbin"):
            ref.fold_check(S, RATE, 2713.7, nbin)
    for f0 in (0.0, -1.0, RATE / (2 * S), float("inf")):
        with pytest.raises(ValueError, match="fold_f0"):
            ref.fold_check(S, RATE, f0, 64)


# ---- bins and the block fold ----

def test_fold_bins_sawtooth():
    nbin, V = 100, 3000
    dphi = T // 777 + 12345
    bins = ref.fold_bins(0, dphi, V, nbin)
    assert bins[0] == 0                       # bin 0 at phase 0
    assert bins.min() == 0 and bins.max() == nbin - 1
    step = np.diff(bins)
    wraps = np.nonzero(step < 0)[0]
    assert (step[step >= 0] <= 1).all()       # 7.77 samples per bin
    assert len(wraps) == (V * dphi) >> 64     # one fall per completed turn
    # just below a turn is the last bin, a turn later bin 0 again
    assert ref.fold_bins(T - 1, 1, 2, nbin).tolist() == [nbin - 1, 0]
    # only the top 32 bits count
    assert ref.fold_bins((1 << 32) - 1, 0, 1, 65536)[0] == 0
    assert ref.fold_bins(1 << 48, 0, 1, 65536)[0] == 1
    # a non power of two: bin = floor(phase * nbin)
    for k, b in enumerate(ref.fold_bins(5, T // 1000, 999, 7)):
        assert b == (5 + k * (T // 1000)) * 7 // T


def test_fold_block_against_a_loop():
    S_, L_, V, nbin = 3, 12, 10, 4
    wf = (np.arange(S_ * L_).reshape(S_, L_) % 7 - 3
          + 1j * (np.arange(S_ * L_).reshape(S_, L_) % 5 - 2)
          ).astype(np.complex64)
    phi, dphi = T - (T // 8), T // 3 + 5
    bins = ref.fold_bins(phi, dphi, V, nbin)
    flags = np.array([0, 1, 0], dtype=np.uint8)
    want = np.zeros((S_, nbin))
    want_hits = np.zeros(nbin, dtype=np.uint64)
    for k in range(V):
        b = ((((phi + k * dphi) % T) >> 32) * nbin) >> 32
        want_hits[b] += 1
        for c in (0, 2):
            want[c, b] += wf[c, k].real ** 2 + wf[c, k].imag ** 2
    got, hits = ref.fold_block(wf, V, bins, nbin, flags)
    assert np.array_equal(got, want) and np.array_equal(hits, want_hits)
    assert got.dtype == np.float64 and hits.dtype == np.uint64
    assert not got[1].any() and got[0].any()
    assert wf[:, V:].any()  # columns beyond V exist and are ignored
    with pytest.raises(ValueError):
        ref.fold_block(wf, L_ + 1, bins, nbin)


def test_cpu_folder_accumulates_blocks():
    S_, N_, r = 4, 4 * 2 * 16, 2 * 4 * 3
    rng = np.random.default_rng(1)
    wf = (rng.integers(-9, 9, (S_, 16)) + 1j * rng.integers(-9, 9, (S_, 16))
          ).astype(np.complex64)
    fo = ref.CpuFolder(N_, r, S_, 1e3, 7.3, 0.0, 0.1, 5)
    V = (N_ - r) // (2 * S_)
    want = np.zeros((S_, 5))
    for i in range(3):
        n0, phi, dphi = fo.add(wf, np.array([0, 0, 1, 0]))
        assert n0 == i * (N_ - r)
        assert (phi, dphi) == ref.fold_phase_words(n0, N_, r, S_, 1e3, 7.3,
                                                   0.0, 0.1)
        a, _ = ref.fold_block(wf, V, ref.fold_bins(phi, dphi, V, 5), 5,
                              np.array([0, 0, 1, 0]))
        want += a
    acc, hits, weights = fo.read()
    assert np.array_equal(acc, want)
    assert hits.sum() == 3 * V
    assert weights.tolist() == [3 * V, 3 * V, 0, 3 * V]
    fo.reset()
    assert fo.next_sample == 3 * (N_ - r) and not fo.read()[0].any()
    with pytest.raises(ValueError):
        ref.CpuFolder(N_, r + 2, S_, 1e3, 7.3, 0.0, 0.1, 5)


# ---- config ----

def test_python_config_keys(tmp_path):
    cfg = Config()
    assert (cfg.fold_output_path, cfg.fold_nbin, cfg.fold_subint_blocks,
            cfg.fold_period_derivative, cfg.fold_phase_offset) == (
        "", 256, 0, 0.0, 0.0)
    path = tmp_path / "c.cfg"
    path.write_text("fold_output_path = /tmp/prof  # stem\n"
                    "fold_period = 455e-3\n"
                    "fold_period_derivative = 2e-14\n"
                    "fold_nbin = 2 ** 10\n")
    cfg = parse_config_file(str(path))
    assert cfg.fold_output_path == "/tmp/prof"
    assert (cfg.fold_period, cfg.fold_nbin) == (0.455, 1024)
    cfg = parse_args(["--config_file_name", str(path), "--fold_phase_offset",
                      "0.25", "--fold_subint_blocks=8"])
    assert (cfg.fold_phase_offset, cfg.fold_subint_blocks) == (0.25, 8)
    f0, f1 = cfg.fold_spin()
    assert f0 == 1 / 0.455 and f1 == -2e-14 / (0.455 * 0.455)
    with pytest.raises(ValueError, match="fold_period"):
        Config().fold_spin()


def test_main_rejects_bad_fold_config(tmp_path):
    from srtb_amd.main import main
    base = ["--device", "cpu", "--input_file_path", "/nonexistent",
            "--fold_output_path", str(tmp_path / "p")]
    with pytest.raises(SystemExit) as e:
        main(base + ["--fold_period", "0.4", "--dm_trial_list", "0, 60"])
    assert "fold_output_path" in str(e.value) and "dm_trial_list" in str(e.value)
    with pytest.raises(SystemExit, match="fold_period"):
        main(base)
    with pytest.raises(SystemExit, match="fold_nbin"):
        main(base + ["--fold_period", "0.4", "--fold_nbin", "1"])
    with pytest.raises(SystemExit, match="fold_f0"):
        main(base + ["--fold_period", "1e-9"])


def dry_run(*args):
    return subprocess.run([BIN, "--dry-run", *args], capture_output=True,
                          text=True, timeout=60)


def keyed(stdout):
    return dict(line.split(" = ", 1) for line in stdout.splitlines()
                if " = " in line)


needs_bin = pytest.mark.skipif(not os.path.exists(BIN),
                               reason="native binaries not built")


@needs_bin
def test_native_dry_run_echoes_fold_keys():
    out = dry_run()
    assert out.returncode == 0, out.stderr
    assert "fold" not in out.stdout
    out = dry_run("--fold_output_path", "/tmp/prof", "--fold_period",
                  "455e-3", "--fold_period_derivative", "2e-14",
                  "--fold_nbin", "2**10", "--fold_phase_offset", "0.25",
                  "--fold_subint_blocks", "8")
    assert out.returncode == 0, out.stderr
    k = keyed(out.stdout)
    assert k["fold_output_path"] == "/tmp/prof"
    assert float(k["fold_period"]) == 0.455
    assert float(k["fold_period_derivative"]) == 2e-14
    assert int(k["fold_nbin"]) == 1024
    assert float(k["fold_phase_offset"]) == 0.25
    assert int(k["fold_subint_blocks"]) == 8
    k = keyed(dry_run("--fold_output_path", "/tmp/prof", "--fold_period",
                      "0.455").stdout)
    assert (int(k["fold_nbin"]), int(k["fold_subint_blocks"])) == (256, 0)


@needs_bin
def test_native_overlap_rule_with_fold():
    """Folding needs whole waterfall columns only, which the overlap already
    leaves: the path changes nothing, alone or next to the filterbank."""
    n, s, t = 1 << 24, 1 << 8, 16
    args = ["--baseband_input_count", str(n), "--spectrum_channel_count",
            str(s), "--baseband_freq_low", "1437", "--baseband_bandwidth",
            "-64", "--baseband_sample_rate", "128e6", "--dm", "-56.77",
            "--input_file_path", "/nonexistent"]
    fold = ["--fold_output_path", "/tmp/prof", "--fold_period", "0.455"]
    fil = ["--filterbank_output_path", "/tmp/a.fil", "--filterbank_tscrunch",
           str(t)]
    on = int(keyed(dry_run(*args, *fold).stdout)["nsamps_reserved"])
    both = int(keyed(dry_run(*args, *fold, *fil).stdout)["nsamps_reserved"])
    assert on == ref.nsamps_reserved(n, s, 1437.0, -64.0, 128e6, -56.77)
    assert both == ref.nsamps_reserved(n, s, 1437.0, -64.0, 128e6, -56.77,
                                       time_multiple=t)
    assert 0 < on < n and (n - on) % (2 * s) == 0


@needs_bin
def test_native_rejects_bad_fold_config():
    out = dry_run("--fold_output_path", "/tmp/prof", "--fold_period", "0.455",
                  "--dm_trial_list", "0, 60")
    assert out.returncode != 0
    text = out.stderr + out.stdout
    assert "dm_trial_list" in text and "fold_output_path" in text
    for extra, word in [([], "fold_period"),
                        (["--fold_period", "0.455", "--fold_nbin", "1"],
                         "fold_nbin"),
                        (["--fold_period", "1e-9"], "fold_period")]:
        out = dry_run("--fold_output_path", "/tmp/prof", *extra)
        assert out.returncode != 0
        assert word in out.stderr + out.stdout


# ---- srtb_amd.main --device cpu end to end ----

PERIOD_SAMPLES = 47371.3          # incommensurate with the block, 0.37 ms
PERIOD = PERIOD_SAMPLES / RATE
PULSE_PHASE = 0.3047              # turns: the middle of bin 19 of 64
NBIN = 64
PEAK_BIN = int(PULSE_PHASE * NBIN)


def pulse_train(n_total, amp=100.0):
    """One-sample pulses (flat across the band) at (j + PULSE_PHASE) periods."""
    x = np.zeros(n_total)
    j = np.arange(int(n_total / PERIOD_SAMPLES) + 1)
    idx = np.round((j + PULSE_PHASE) * PERIOD_SAMPLES).astype(np.int64)
    x[idx[idx < n_total]] = amp
    return x


def to_int8(x, seed):
    rng = np.random.default_rng(seed)
    return np.clip(np.round(x + rng.normal(0, 2, x.size)), -128,
                   127).astype(np.int8).view(np.uint8)


def train_recording(path, n_blocks=4):
    """DM 0: n_blocks whole blocks, no overlap."""
    to_int8(pulse_train(n_blocks * N), 0).tofile(path)


def dispersed_train_recording(path, dm, n_blocks=4):
    """The same train dispersed at ``dm`` over the whole recording in one
    FFT; n_blocks blocks when read with the seek-back overlap."""
    reserved = ref.nsamps_reserved(N, S, 1400.0, 64.0, RATE, dm)
    assert 0 < reserved < N // 2
    total = N + (n_blocks - 1) * (N - reserved)
    X = np.fft.rfft(pulse_train(total))
    nc = total // 2
    fac = ref.dedisp_phase_factors(nc, 1400.0, 1464.0, 64.0 / nc, dm)
    X[:-1] *= np.conj(fac.astype(np.complex128))
    to_int8(np.fft.irfft(X, total), 1).tofile(path)
    return reserved


APP_ARGS = [
    "--baseband_input_count", str(N), "--baseband_input_bits", "-8",
    "--spectrum_channel_count", str(S), "--baseband_freq_low", "1400",
    "--baseband_bandwidth", "64", "--baseband_sample_rate", "128e6",
    "--mitigate_rfi_average_method_threshold", "1e30",
    "--mitigate_rfi_spectral_kurtosis_threshold", "1e30",
    "--signal_detect_signal_noise_threshold", "1e30",
    "--signal_detect_max_boxcar_length", "16",
    "--fold_period", repr(PERIOD), "--fold_nbin", str(NBIN),
    "--fold_subint_blocks", "2",
]


def load_subint(stem, index):
    p = fold_subint_paths(str(stem), index)
    for f in p.values():
        assert os.path.exists(f), f
    return (np.load(p["profile"]), np.load(p["hits"]), np.load(p["weights"]),
            read_fold_meta(p["meta"]))


def check_profile(acc, hits, V_blocks):
    """Peak at the predicted bin +-1, at least 80 % of the power above the
    median within +-1 bin of the peak, hits complete."""
    assert acc.shape == (S, NBIN) and acc.dtype == np.float64
    assert hits.dtype == np.uint64 and int(hits.sum()) == V_blocks
    prof = acc.sum(axis=0) / hits
    peak = int(np.argmax(prof))
    assert abs(peak - PEAK_BIN) <= 1, (peak, PEAK_BIN)
    excess = np.clip(prof - np.median(prof), 0, None)
    near = excess[[(peak - 1) % NBIN, peak, (peak + 1) % NBIN]].sum()
    print("peak", peak, "concentration", near / excess.sum())
    assert near >= 0.8 * excess.sum()


def test_main_cpu_folds_a_pulse_train(tmp_path):
    from srtb_amd.main import main
    rec = tmp_path / "rec.bin"
    train_recording(rec)
    stem = tmp_path / "prof"
    rc = main(APP_ARGS + [
        "--device", "cpu", "--dm", "0", "--input_file_path", str(rec),
        "--fold_output_path", str(stem),
        "--baseband_output_file_prefix", str(tmp_path) + "/p_"])
    assert rc == 0
    V = N // (2 * S)
    for i in range(2):
        acc, hits, weights, meta = load_subint(stem, i)
        check_profile(acc, hits, 2 * V)
        assert weights.dtype == np.uint64 and (weights == 2 * V).all()
        assert int(meta["first_sample"]) == i * 2 * N
        assert int(meta["n_blocks"]) == 2 and int(meta["nbin"]) == NBIN
        assert float(meta["f0"]) == 1.0 / PERIOD and float(meta["f1"]) == 0.0
        assert float(meta["tsamp"]) == 2 * S / RATE
        assert float(meta["dm"]) == 0.0 and "row" in meta["row_order"]
    assert not os.path.exists(fold_subint_paths(str(stem), 2)["profile"])


def test_main_cpu_folds_across_the_overlap(tmp_path):
    """DM ~ 1: blocks overlap by 0 < nsamps_reserved < N / 2 and advance by
    N - nsamps_reserved.  A fold advancing by N would smear the pulse over
    (reserved / PERIOD_SAMPLES) turns per block."""
    from srtb_amd.main import main
    rec = tmp_path / "rec.bin"
    reserved = dispersed_train_recording(rec, 1.0)
    assert abs((reserved / PERIOD_SAMPLES) % 1 - 0.5) < 0.49  # not a whole turn
    stem = tmp_path / "prof"
    rc = main(APP_ARGS + [
        "--device", "cpu", "--dm", "1.0", "--input_file_path", str(rec),
        "--fold_output_path", str(stem),
        "--baseband_output_file_prefix", str(tmp_path) + "/p_"])
    assert rc == 0
    V = (N - reserved) // (2 * S)
    for i in range(2):
        acc, hits, weights, meta = load_subint(stem, i)
        check_profile(acc, hits, 2 * V)
        assert int(meta["first_sample"]) == i * 2 * (N - reserved)
