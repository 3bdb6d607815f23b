"""GPU tests of the flagship benchmark's command line (bench.py)."""

import glob
import json
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

CHANNELS = 1 << 8
BLOCKS = 2


def run_bench(monkeypatch, capsys, *args):
    import bench
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", *args])
    bench.main()
    return json.loads(capsys.readouterr().out.strip().splitlines()[-1])


def load_dump(d):
    return {os.path.basename(f)[:-4]: np.load(f)
            for f in sorted(glob.glob(os.path.join(str(d), "*.npy")))}


# 2^20: the waterfall (2^19 complex) is dumped whole; 2^23: the waterfall
# (2^22 complex = 32 MiB) exceeds DUMP_WATERFALL_BYTES and is sampled
@pytest.mark.parametrize("log2n", [20, 23])
def test_dump_outputs(tmp_path, monkeypatch, capsys, log2n):
    import bench
    n = 1 << log2n
    common = ["--steps", "2", "--warmup", "1", "--input-count", str(n),
              "--channels", str(CHANNELS), "--blocks-per-step", str(BLOCKS)]
    outs = []
    for name in ("a", "b"):
        d = run_bench(monkeypatch, capsys, *common,
                      "--dump-outputs", str(tmp_path / name))
        assert d["steps"] == 2 and d["ms_per_step"] > 0 and d["value"] > 0
        outs.append(load_dump(tmp_path / name))
    a, b = outs

    n_complex = n // 2
    k = min(n_complex, bench.DUMP_WATERFALL_BYTES // 8)
    sampled = n_complex > k
    names = {"detect_counts", "detect_boxcars", "detect_thresholds",
             "time_series", "waterfall"} | ({"waterfall_index"} if sampled
                                            else set())
    assert set(a) == names
    assert sum(x.nbytes for x in a.values()) <= 64 * 10**6
    for x in a.values():
        assert x.dtype in (np.float32, np.float64)
        assert np.isfinite(x).all()
    n_box = a["detect_boxcars"].size
    assert n_box > 0 and a["detect_boxcars"][0] == 1
    assert a["detect_counts"].shape == (BLOCKS, 1 + n_box)
    assert a["detect_thresholds"].shape[0] == BLOCKS
    assert a["time_series"].ndim == 1 and a["time_series"].size > 0
    assert a["waterfall"].shape == (k, 2)
    assert np.count_nonzero(a["waterfall"]) > 0
    if sampled:
        idx = a["waterfall_index"]
        assert idx.shape == (k,)
        assert idx.min() >= 0 and idx.max() < n_complex
        assert (np.diff(idx) >= 0).all()

    # same arguments -> same inputs -> same outputs, run to run
    for name in names:
        np.testing.assert_array_equal(a[name], b[name], err_msg=name)


def test_full_flag_keeps_result_line(monkeypatch, capsys):
    d = run_bench(monkeypatch, capsys, "--steps", "1", "--warmup", "1",
                  "--input-count", str(1 << 20), "--channels", str(CHANNELS),
                  "--blocks-per-step", "1", "--full")
    for key in ("metric", "value", "unit", "higher_is_better", "dtype",
                "ms_per_step"):
        assert key in d
    assert d["unit"] == "Msamples/s" and d["higher_is_better"] is True
    assert d["steps"] == 1
