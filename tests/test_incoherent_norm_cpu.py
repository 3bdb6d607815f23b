"""CPU tests of the per-channel normalisation before the incoherent DM-offset
search: the oracle's block statistics, the running state of
CpuIncoherentSearch, the two configuration keys and srtb_amd.main on the CPU.

The loud-channel input set below is shared with tests/test_gpu_incoherent_norm.
"""

import numpy as np
import pytest

from srtb_amd import ref
from srtb_amd.config import Config, parse_args

# ---- the loud-channel input set ----

LOUD = dict(R=64, C=96, fch1=1500.0, foff=-1.0, tsamp=1e-3,
            offsets=[-100.0, -50.0, 0.0, 50.0, 100.0], snr_threshold=6.0,
            max_boxcar=4)
LOUD_BLOCKS = 8
LOUD_CHANNELS = [5, 40, 77]
# the one candidate with the feature on: block, offset, boxcar length, global
# row of the peak
LOUD_CANDIDATE = (5, 50.0, 1, 5 * 64 + 10)


def loud_channel_planes():
    """8 blocks of gamma(16, 1) noise [64][96]; channels 5, 40 and 77 are 300
    times as loud; a pulse of +12 in every other channel, swept at delta = 50
    from global row 330."""
    kw = dict(LOUD)
    R, C = kw["R"], kw["C"]
    x = np.random.default_rng(7).gamma(16, 1, (LOUD_BLOCKS * R, C)).astype(
        np.float32)
    x[:, LOUD_CHANNELS] *= np.float32(300)
    d = ref.incoherent_delays(kw["fch1"], kw["foff"], C, kw["tsamp"],
                              [50.0])[0]
    quiet = np.setdiff1d(np.arange(C), LOUD_CHANNELS)
    x[LOUD_CANDIDATE[3] + d[quiet], quiet] += np.float32(12)
    return [x[b * R:(b + 1) * R] for b in range(LOUD_BLOCKS)]


def cpu_search(**over):
    kw = dict(LOUD)
    kw.update(over)
    return ref.CpuIncoherentSearch(kw.pop("R"), kw.pop("C"), **kw)


def all_detections(results):
    """[(snr, count, block, offset, length, global row)] of every valid
    (trial, length) of a list of result dicts."""
    out = []
    for res in results:
        for tr in res["trials"]:
            for ln in tr["lengths"]:
                out.append((ln["snr"], ln["count"], res["block"],
                            tr["offset"], ln["boxcar_length"],
                            res["first_row"] + ln["index"]))
    return out


def candidates_of(results):
    return [d for d in all_detections(results) if d[1] > 0]


# ---- block statistics ----

@pytest.mark.parametrize("R,C", [(2, 1), (64, 96), (67, 37), (130, 1028)])
def test_stats_match_numpy(R, C):
    rng = np.random.default_rng(R * 1000 + C)
    P = rng.gamma(16, 1, (R, C)).astype(np.float32)
    m, v = ref.incoherent_norm_stats(P)
    assert m.dtype == np.float64 and v.dtype == np.float64
    assert m.shape == (C,) and v.shape == (C,)
    P64 = P.astype(np.float64)
    want_m, want_v = P64.mean(axis=0), P64.var(axis=0)
    # the first sample lies within 6 sigma: the bounds of the GPU test
    assert (np.abs(P64[0] - want_m) <= 6 * np.sqrt(want_v) + 1e-300).all()
    assert (np.abs(m - want_m) <= (R + 1) * 2.0 ** -53 * np.abs(want_m)).all()
    assert (np.abs(v - want_v) <= 40 * (R + 1) * 2.0 ** -53 * want_v).all()


def test_stats_are_exact_on_small_integers():
    rng = np.random.default_rng(1)
    P = rng.integers(0, 16, (64, 37)).astype(np.float32)
    m, v = ref.incoherent_norm_stats(P)
    s = P.astype(np.int64).sum(axis=0)
    s2 = (P.astype(np.int64) ** 2).sum(axis=0)
    assert np.array_equal(m, s / 64.0)
    assert np.array_equal(v, (64 * s2 - s * s) / 4096.0)


def test_a_constant_channel_has_no_variance_and_no_gain():
    rng = np.random.default_rng(2)
    P = rng.gamma(16, 1, (67, 5)).astype(np.float32)
    P[:, 1] = np.float32(1234.5678)  # not exactly representable sums
    P[:, 3] = 0
    m, v = ref.incoherent_norm_stats(P)
    assert v[1] == 0.0 and v[3] == 0.0 and (v[[0, 2, 4]] > 0).all()
    assert m[1] == np.float64(np.float32(1234.5678)) and m[3] == 0.0
    G = ref.incoherent_norm_gain(v)
    assert G.dtype == np.float32
    assert G[1] == 0 and G[3] == 0 and (G[[0, 2, 4]] > 0).all()
    out = ref.incoherent_norm_apply(P, m, G)
    assert out.dtype == np.float32
    assert (out[:, [1, 3]] == 0).all()


# ---- the running state ----

def test_alpha_is_cumulative_then_exponential():
    """With a plane of the constant-per-block value x_b in channel 0 the
    block mean is x_b exactly, so M follows alpha = 1, 1/2, ... 1/K, 1/K."""
    K, R, C = 3, 4, 2
    s = ref.CpuIncoherentSearch(R, C, 1500.0, -1.0, 1e-3, [0.0], 6.0, 1,
                                normalize=True, normalize_blocks=K)
    rng = np.random.default_rng(3)
    M = np.float64(0.0)
    V = np.float64(0.0)
    alphas = []
    for b in range(7):
        x = np.float32(rng.integers(1, 100))
        P = np.empty((R, C), dtype=np.float32)
        P[:, 0] = x
        P[:, 1] = [x, x + 2, x, x + 2]  # mean x + 1, variance 1
        res = s.add(P)
        alpha = np.float64(1.0) / np.float64(min(b + 1, K))
        alphas.append(alpha)
        M = M + alpha * (np.float64(x) - M)
        V = V + alpha * (np.float64(1.0) - V)
        assert s.M[0] == M and s.V[0] == 0.0 and s.G[0] == 0
        assert s.V[1] == V
        assert res["live_channels"] == 1
    assert alphas[:4] == [1.0, 0.5, 1.0 / 3.0, 1.0 / 3.0]
    assert s.V[1] == 1.0  # every block had variance 1


def test_the_first_block_is_normalised_by_its_own_statistics():
    planes = loud_channel_planes()
    s = cpu_search(normalize=True)
    s.add(planes[0])
    m, v = ref.incoherent_norm_stats(planes[0])
    assert np.array_equal(s.M, m) and np.array_equal(s.V, v)
    newest = s.window[-LOUD["R"]:]
    assert np.array_equal(
        newest, ref.incoherent_norm_apply(planes[0], m, s.G))
    assert (np.abs(newest.mean(axis=0)) < 1e-5).all()
    assert (np.abs(newest.std(axis=0) - 1) < 1e-5).all()


def test_reset_restarts_the_state():
    planes = loud_channel_planes()
    a, b = cpu_search(normalize=True), cpu_search(normalize=True)
    for p in planes[:3]:
        a.add(p)
    a.reset()
    assert not a.M.any() and not a.V.any() and not a.G.any()
    for p in planes[3:6]:
        ra, rb = a.add(p), b.add(p)
        assert ra["block"] == rb["block"]
        assert ra["live_channels"] == rb["live_channels"] == LOUD["C"]
        assert np.array_equal(ra["Y"], rb["Y"])
        assert np.array_equal(a.M, b.M) and np.array_equal(a.V, b.V)


def test_normalize_off_is_the_search_as_it_was():
    """The defaults, normalize=False, and the sum written out by hand."""
    rng = np.random.default_rng(4)
    R, C = 8, 16
    args = (R, C, 1463.5, -4.0, 2.5e-4, [-30.0, 0.0, 12.5, 40.0], 2.0, 4)
    plain = ref.CpuIncoherentSearch(*args)
    off = ref.CpuIncoherentSearch(*args, normalize=False, normalize_blocks=3)
    planes = [rng.normal(10.0, 3.0, (R, C)).astype(np.float32)
              for _ in range(6)]
    stream = np.concatenate([np.zeros((plain.d_max, C))] + planes)
    whole = ref.incoherent_dedisperse(stream, plain.delays, 6 * R)
    for b, p in enumerate(planes):
        r0, r1 = plain.add(p), off.add(p)
        assert np.array_equal(r0["Y"], whole[:, b * R:(b + 1) * R])
        assert np.array_equal(r0["Y"], r1["Y"])
        assert r0["trials"] == r1["trials"]
        assert r0["live_channels"] == r1["live_channels"] == 0
        assert (r0["valid"], r0["first_row"], r0["block"]) == \
            (r1["valid"], r1["first_row"], r1["block"])


def test_constructor_rejects_k_out_of_range():
    for K in (0, -1, 65537):
        with pytest.raises(ValueError, match="normalize_blocks"):
            cpu_search(normalize=True, normalize_blocks=K)
        with pytest.raises(ValueError, match="normalize_blocks"):
            cpu_search(normalize_blocks=K)
    cpu_search(normalize=True, normalize_blocks=1)
    cpu_search(normalize=True, normalize_blocks=65536)


# ---- the loud-channel case ----

def test_loud_channels_hide_the_pulse_until_normalised():
    """The margins the GPU tests rely on, from the oracle itself: measured
    snr 7.61 for the candidate with the feature on, every other (trial,
    length) of every block below 5.5; best snr 3.93 with the feature off."""
    planes = loud_channel_planes()
    s_on, s_off = cpu_search(normalize=True), cpu_search()
    on = [s_on.add(p) for p in planes]
    off = [s_off.add(p) for p in planes]
    assert [r["valid"] for r in on] == [r["valid"] for r in off]
    assert all(r["live_channels"] == LOUD["C"] for r in on)

    assert candidates_of(off) == []
    print("off: best snr", max(d[0] for d in all_detections(off)))
    assert max(d[0] for d in all_detections(off)) < 5.5

    cands = candidates_of(on)
    assert len(cands) == 1
    snr, count, block, offset, length, row = cands[0]
    print("on: candidate", cands[0])
    assert (block, offset, length, row) == LOUD_CANDIDATE and count == 1
    assert snr > 6.5
    others = sorted(d[0] for d in all_detections(on) if d[2:] != cands[0][2:])
    print("on: next best snr", others[-1])
    assert others[-1] < 5.5


# ---- configuration ----

def test_config_defaults_and_parsing():
    cfg = Config()
    assert cfg.incoherent_normalize is False
    assert cfg.incoherent_normalize_blocks == 8
    cfg = parse_args(["--incoherent_normalize", "1",
                      "--incoherent_normalize_blocks", "2 ** 4"])
    assert cfg.incoherent_normalize is True
    assert cfg.incoherent_normalize_blocks == 16
    assert parse_args(["--incoherent_normalize", "0"]).incoherent_normalize \
        is False


def app_args():
    from tests.test_incoherent_cpu import APP_ARGS
    return APP_ARGS


def test_main_rejects_normalize_without_offsets():
    from srtb_amd.main import main
    base = app_args() + ["--device", "cpu", "--input_file_path", "none.bin"]
    with pytest.raises(SystemExit, match="incoherent_normalize needs "
                                         "incoherent_dm_offsets"):
        main(base + ["--incoherent_normalize", "1"])


@pytest.mark.parametrize("K", ["0", "65537", "-3"])
def test_main_rejects_k_out_of_range(tmp_path, K):
    from srtb_amd.main import main
    base = app_args() + ["--device", "cpu", "--input_file_path", "none.bin",
                         "--incoherent_dm_offsets", "0,1",
                         "--incoherent_output_path", str(tmp_path / "c.cand")]
    with pytest.raises(SystemExit, match="incoherent_normalize_blocks must "
                                         "be 1 .. 65536"):
        main(base + ["--incoherent_normalize", "1",
                     "--incoherent_normalize_blocks", K])


def test_main_cpu_normalised_run(tmp_path):
    """The recording of test_incoherent_cpu through main --device cpu with
    the key at 1 and at 0: both find the injected offset, and the candidates
    differ (every snr is that of normalised rows)."""
    from srtb_amd.main import main
    from tests.test_incoherent_cpu import (check_candidates,
                                           offset_pulse_recording)
    rec = tmp_path / "rec.bin"
    offset_pulse_recording(rec)
    outs = {}
    for key in ("1", "0"):
        out = tmp_path / f"n{key}.cand"
        rc = main(app_args() + [
            "--device", "cpu", "--input_file_path", str(rec),
            "--incoherent_dm_offsets", "-2,-1,0,1,2,3,4",
            "--incoherent_output_path", str(out),
            "--incoherent_normalize", key,
            "--incoherent_normalize_blocks", "4",
            "--baseband_output_file_prefix", f"{tmp_path}/o{key}_"])
        assert rc == 0
        check_candidates(out)
        outs[key] = out.read_bytes()
    assert outs["1"] != outs["0"]
    # the key at 0 is the run without the keys
    plain = tmp_path / "plain.cand"
    assert main(app_args() + [
        "--device", "cpu", "--input_file_path", str(rec),
        "--incoherent_dm_offsets", "-2,-1,0,1,2,3,4",
        "--incoherent_output_path", str(plain),
        "--baseband_output_file_prefix", f"{tmp_path}/op_"]) == 0
    assert plain.read_bytes() == outs["0"]
