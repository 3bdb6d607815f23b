"""The dm_trial_list key, without a GPU: the native --dry-run and the Python
Config twin."""

import os
import subprocess

import pytest

from srtb_amd import ref
from srtb_amd.config import Config, parse_args, parse_config_file

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BACKEND = os.path.join(ROOT, "bin", "srtb-backend")

needs_bins = pytest.mark.skipif(not os.path.exists(BACKEND),
                                reason="native binaries not built")


def dry_run(*args):
    return subprocess.run([BACKEND, "--dry-run", *args], capture_output=True,
                          text=True, timeout=30)


def keyed(stdout):
    return dict(l.split(" = ", 1) for l in stdout.strip().splitlines()
                if " = " in l)


@needs_bins
def test_dry_run_echoes_evaluated_trial_list():
    out = dry_run("--dm_trial_list", "2**3, 56.77")
    assert out.returncode == 0, out.stderr
    got = [float(x) for x in keyed(out.stdout)["dm_trial_list"].split(",")]
    assert got == [8.0, 56.77]


@needs_bins
def test_dry_run_reads_trial_list_from_file(tmp_path):
    cfg = tmp_path / "c.cfg"
    cfg.write_text("dm = 10\ndm_trial_list = 0, 10 * 2, sqrt(16)  # trials\n")
    out = dry_run("--config_file_name", str(cfg))
    assert out.returncode == 0, out.stderr
    got = [float(x) for x in keyed(out.stdout)["dm_trial_list"].split(",")]
    assert got == [0.0, 20.0, 4.0]


@needs_bins
def test_dry_run_without_trial_list_prints_no_such_line():
    out = dry_run("--dm", "60")
    assert out.returncode == 0, out.stderr
    assert "dm_trial_list" not in out.stdout


@needs_bins
@pytest.mark.parametrize("dm,trials,largest", [
    ("0", "0, 20, 120, 56.77", 120.0),      # a trial sets the overlap
    ("-478.8", "-100, 30", -478.8),         # the configured dm still counts
])
def test_dry_run_overlap_covers_largest_trial(dm, trials, largest):
    n, s = 2**25, 2**11
    bw = 64.0 if largest > 0 else -64.0
    f_low = 1400.0 if largest > 0 else 1437.0
    out = dry_run("--baseband_input_count", str(n),
                  "--spectrum_channel_count", str(s),
                  "--baseband_freq_low", str(f_low),
                  "--baseband_bandwidth", str(bw),
                  "--baseband_sample_rate", "128e6", "--dm", dm,
                  "--dm_trial_list", trials, "--baseband_reserve_sample", "1")
    assert out.returncode == 0, out.stderr
    got = int(out.stdout.strip().splitlines()[-1].split(" = ")[1])
    expect = ref.nsamps_reserved(n, s, f_low, bw, 128e6, largest)
    assert expect > 0
    assert got == expect


@needs_bins
def test_dry_run_rejects_trial_list_with_two_polarisations():
    out = dry_run("--baseband_format_type", "naocpsr_snap1",
                  "--dm_trial_list", "0, 60")
    assert out.returncode != 0
    assert "dm_trial_list" in out.stderr + out.stdout
    # the format alone is fine
    assert dry_run("--baseband_format_type",
                   "naocpsr_snap1").returncode == 0


@needs_bins
def test_dry_run_rejects_malformed_trial_list():
    out = dry_run("--dm_trial_list", "0, sixty")
    assert out.returncode != 0


def test_config_parses_trial_list_from_file_and_command_line(tmp_path):
    assert Config().dm_trial_list == ""
    assert Config().dm_trials() == []
    path = tmp_path / "c.cfg"
    path.write_text("dm_trial_list = 2**3, 56.77  # Crab\n")
    cfg = parse_config_file(str(path))
    assert cfg.dm_trials() == [8.0, 56.77]
    cfg = parse_args(["--config_file_name", str(path),
                      "--dm_trial_list", "0, 10*2,sqrt(16)"])
    assert cfg.dm_trials() == [0.0, 20.0, 4.0]
    cfg = parse_args(["--dm_trial_list=-478.8"])
    assert cfg.dm_trials() == [-478.8]
    assert cfg.copy().dm_trials() == [-478.8]


@pytest.mark.parametrize("bad", ["1,,2", "0, sixty", "1 2", "3,"])
def test_config_rejects_malformed_trial_list(bad):
    with pytest.raises(ValueError):
        Config().assign("dm_trial_list", bad)
