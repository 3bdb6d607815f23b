"""GPU tests of pulsar folding: the stand-alone fold kernels (bitwise, on
integer waterfalls whose sums are exact in float32), the engine path with its
phase bookkeeping across blocks, slots and hipGraph replay, and both apps
writing sub-integration files.

Oracle: srtb_amd.ref.fold_phase_words / fold_bins / fold_block in Python
integers and float64, fed with the GPU's own waterfall in the engine tests.
"""

import os
import subprocess

import numpy as np
import pytest
import torch

from srtb_amd import ref
from srtb_amd.config import Config
from srtb_amd.pipeline.cpu import synthesize_dispersed_pulse

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "bin", "srtb-backend")

N, S = 1 << 18, 1 << 6
L = N // 2 // S
ZAP = [[100, 300]]
TONE_ROW = 20  # waterfall row the sweeping tone sits in
RATE = 128e6
F0 = 2713.7    # Hz: 5.56 turns per block of 2048 waterfall samples of 1 us
PHASE0 = 0.3


@pytest.fixture(scope="module")
def C():
    from srtb_amd.ops import native
    torch.cuda.set_device(0)
    return native()


def make_engine(C, fft=0, **kw):
    args = dict(
        n=N, nbits=-8, channels=S, freq_low=1400.0, bandwidth=64.0,
        sample_rate=RATE, dm=60.0, rfi_threshold=20.0, sk_threshold=1.5,
        snr_threshold=6.0, max_boxcar=16, nsamps_reserved=0, zap_ranges=ZAP,
        use_phase_table=False, enable_rfi_s1=True, enable_sk=True, n_slots=2,
        fft_backend=fft)
    args.update(kw)
    return C.PipelineEngine(**args)


def fold_kw(nbin=64, f0=F0, f1=0.0, phase0=PHASE0):
    return dict(fold_nbin=nbin, fold_f0=f0, fold_f1=f1, fold_phase0=phase0)


def make_block(seed=0):
    """int8 noise (sigma 16) + a constant-envelope tone sweeping across
    waterfall row 20 during the block (spectral kurtosis ~1.35: the row is
    flagged; spread over 2048 bins it stays below the RFI-s1 threshold, which
    a pure CW tone would not) + one band-filling pulse at DM 60 of about 20
    times the mean power per channel sample (not flagged, saturates 8 bits)."""
    cfg = Config()
    cfg.baseband_input_count = N
    cfg.spectrum_channel_count = S
    cfg.baseband_input_bits = -8
    cfg.baseband_freq_low = 1400.0
    cfg.baseband_bandwidth = 64.0
    cfg.baseband_sample_rate = RATE
    cfg.dm = 60.0
    raw = synthesize_dispersed_pulse(
        cfg, 0.3 * N / RATE, pulse_amp=7.5, noise_sigma=16.0,
        rng=np.random.default_rng(seed), width=1)
    t = np.arange(N, dtype=np.float64)
    f0, f1 = TONE_ROW * 1e6 / RATE, (TONE_ROW + 1) * 1e6 / RATE
    tone = 10.0 * np.cos(2 * np.pi * (f0 * t + 0.5 * (f1 - f0) * t * t / N))
    x = raw.view(np.int8).astype(np.float64) + np.round(tone)
    return torch.from_numpy(
        np.clip(x, -128, 127).astype(np.int8).view(np.uint8).copy())


@pytest.fixture(scope="module")
def raw():
    return make_block()


# ---- 1. stand-alone kernels, bitwise ----

def pattern_waterfall(S_, L_):
    """Small integers without symmetry in row or time, |.|^2 <= 421."""
    t = np.arange(L_)[None, :]
    r = np.arange(S_)[:, None]
    re = (t * 7 + r * 3) % 31 - 15
    im = (t * 5 + r * 11) % 29 - 14
    return (re + 1j * im).astype(np.complex64)


T = 1 << 64
KERNEL_CASES = [
    # S, L, V, nbin, Phi, dPhi
    (1, 8, 1, 2, 0, 0),                               # the smallest
    (6, 10, 6, 4, T - 1, 1 << 62),                    # wrap at the first step
    (70, 300, 149, 100, 12345 << 40, T // 37 + 1),    # bins skipped
    (5, 4096, 4000, 8, 1 << 63, T // 1000),           # runs of 125 samples
    (3, 2048, 1536, 64, 7, T // 64),                  # one sample per bin
    (2, 8192, 8192, 65536, 0, T // 3001),             # mostly empty bins
    (66, 512, 512, 33, 1 << 61, 0),                   # everything in one bin
    (192, 96, 72, 16, 99, T // 7 - 5),                # S beyond any tile
]


def run_fold_block(C, wf, flags, V, nbin, phi, dphi, out=None):
    S_ = wf.shape[0]
    if out is None:
        out = (torch.zeros(S_, nbin, dtype=torch.float64, device="cuda"),
               torch.zeros(nbin, dtype=torch.int64, device="cuda"),
               torch.zeros(S_, dtype=torch.int64, device="cuda"))
    C.fold_block(torch.from_numpy(wf).cuda(), flags, V, nbin, phi, dphi, *out)
    return out


def to_host(out):
    acc, hits, weights = out
    return (acc.cpu().numpy(), hits.cpu().numpy().view(np.uint64),
            weights.cpu().numpy().view(np.uint64))


@pytest.mark.parametrize("with_flags", [False, True])
@pytest.mark.parametrize("S_,L_,V,nbin,phi,dphi", KERNEL_CASES)
def test_fold_kernel_exact(C, S_, L_, V, nbin, phi, dphi, with_flags):
    wf = pattern_waterfall(S_, L_)
    f = np.zeros(S_, dtype=np.uint8)
    if with_flags:
        f[[0, S_ // 2, S_ - 1]] = 1
    bins = ref.fold_bins(phi, dphi, V, nbin)
    want, want_hits = ref.fold_block(wf, V, bins, nbin, f)
    assert want.max() < 2 ** 24  # every partial sum is exact in float32
    flags = torch.from_numpy(f).cuda() if with_flags else None
    acc, hits, weights = to_host(
        run_fold_block(C, wf, flags, V, nbin, phi, dphi))
    assert np.array_equal(hits, want_hits)
    assert int(hits.sum()) == V
    assert np.array_equal(weights, np.where(f != 0, 0, V).astype(np.uint64))
    assert np.array_equal(acc, want), np.argwhere(acc != want)[:8]
    if not with_flags or S_ > 3:
        assert want.any()


def test_fold_kernel_accumulates(C):
    S_, L_, V, nbin = 70, 300, 149, 100
    wf = pattern_waterfall(S_, L_)
    words = [(12345 << 40, T // 37 + 1), (T - 3, T // 5 + 11)]
    out = None
    want = np.zeros((S_, nbin))
    want_hits = np.zeros(nbin, dtype=np.uint64)
    for phi, dphi in words:
        out = run_fold_block(C, wf, None, V, nbin, phi, dphi, out)
        a, h = ref.fold_block(wf, V, ref.fold_bins(phi, dphi, V, nbin), nbin)
        want += a
        want_hits += h
    acc, hits, weights = to_host(out)
    assert want.max() < 2 ** 24
    assert np.array_equal(acc, want)
    assert np.array_equal(hits, want_hits)
    assert np.array_equal(weights, np.full(S_, 2 * V, dtype=np.uint64))


def test_fold_kernel_rejects_bad_geometry(C):
    wf = torch.zeros(6, 10, dtype=torch.complex64).cuda()

    def out(s_=6, nbin=4, acc_dtype=torch.float64):
        return (torch.zeros(s_, nbin, dtype=acc_dtype, device="cuda"),
                torch.zeros(nbin, dtype=torch.int64, device="cuda"),
                torch.zeros(s_, dtype=torch.int64, device="cuda"))

    with pytest.raises(RuntimeError):  # V > L
        C.fold_block(wf, None, 11, 4, 0, 1, *out())
    with pytest.raises(RuntimeError):  # V = 0
        C.fold_block(wf, None, 0, 4, 0, 1, *out())
    with pytest.raises(RuntimeError):  # nbin too small
        C.fold_block(wf, None, 6, 1, 0, 1, *out(nbin=1))
    with pytest.raises(RuntimeError):  # nbin too large
        C.fold_block(wf, None, 6, 65537, 0, 1, *out(nbin=65537))
    with pytest.raises(RuntimeError):  # acc rows
        C.fold_block(wf, None, 6, 4, 0, 1, *out(s_=5))
    with pytest.raises(RuntimeError):  # acc bins
        a, h, w = out()
        C.fold_block(wf, None, 6, 4, 0, 1, out(nbin=5)[0], h, w)
    with pytest.raises(RuntimeError):  # acc dtype
        C.fold_block(wf, None, 6, 4, 0, 1, *out(acc_dtype=torch.float32))
    with pytest.raises(RuntimeError):  # hits length
        a, h, w = out()
        C.fold_block(wf, None, 6, 4, 0, 1, a, h[:3], w)


# ---- 2. engine ----

def engine_oracle(wf, words, nbin, V):
    """Sum of the fp64 oracle blocks of one (zapped) waterfall at the given
    (n0, Phi, dPhi) words; the weights follow from the zapped rows."""
    acc = np.zeros((wf.shape[0], nbin))
    hits = np.zeros(nbin, dtype=np.uint64)
    per_block_hits = 0
    for _n0, phi, dphi in words:
        a, h = ref.fold_block(wf, V, ref.fold_bins(phi, dphi, V, nbin), nbin)
        acc += a
        hits += h
        per_block_hits = max(per_block_hits, int(h.max()))
    good = np.abs(wf).max(axis=1) > 0
    weights = np.where(good, V * len(words), 0).astype(np.uint64)
    return acc, hits, weights, per_block_hits


def assert_fold_close(got, want, n_terms):
    rtol = (n_terms + 4) * 2.0 ** -23
    err = np.abs(got - want) / np.where(want > 0, want, 1.0)
    print("max rel err", err.max(), "bound", rtol)
    np.testing.assert_allclose(got, want, rtol=rtol, atol=0)


@pytest.mark.parametrize("reserved", [0, 2 * S * 3])
@pytest.mark.parametrize("fft", [0, 1])
@pytest.mark.parametrize("nbin", [64, 100])
def test_engine_one_block_matches_oracle(C, raw, nbin, fft, reserved):
    eng = make_engine(C, fft=fft, nsamps_reserved=reserved, **fold_kw(nbin))
    V = (N - reserved) // (2 * S)
    slot = eng.submit(raw)
    res = eng.wait(slot)
    assert res["zero_count"] > 0
    acc, hits, weights = eng.fold_read()
    assert acc.dtype == np.float64 and acc.shape == (S, nbin)
    assert hits.dtype == np.uint64 and weights.dtype == np.uint64
    words = eng.fold_words(slot)
    assert words == (0,) + ref.fold_phase_words(0, N, reserved, S, RATE, F0,
                                                0.0, PHASE0)
    # read after the fold: this applies the deferred zap
    wf = eng.waterfall(slot).cpu().numpy()
    want, want_hits, want_w, n_terms = engine_oracle(wf, [words], nbin, V)
    assert np.array_equal(hits, want_hits)
    assert int(hits.sum()) == V
    assert np.array_equal(weights, want_w)
    assert_fold_close(acc, want, n_terms)
    assert (want > 0).any()
    assert (acc[TONE_ROW] == 0).all() and weights[TONE_ROW] == 0
    assert (weights == V).any()


def test_engine_words_follow_the_stream(C, raw):
    reserved = 2 * S * 3
    eng = make_engine(C, nsamps_reserved=reserved, **fold_kw(64))
    fresh = N - reserved

    def want(n0):
        return (n0,) + ref.fold_phase_words(n0, N, reserved, S, RATE, F0, 0.0,
                                            PHASE0)

    assert eng.fold_next_sample() == 0
    for i in range(3):
        slot = eng.submit(raw)
        assert eng.fold_words(slot) == want(i * fresh)
        eng.wait(slot)
    assert eng.fold_next_sample() == 3 * fresh
    eng.set_fold_next_sample(10 ** 12 + 1)
    slot = eng.submit(raw)
    assert eng.fold_words(slot) == want(10 ** 12 + 1)
    eng.wait(slot)
    assert eng.fold_next_sample() == 10 ** 12 + 1 + fresh


def run_three(C, raw, nbin):
    eng = make_engine(C, **fold_kw(nbin))
    words = []
    s0 = eng.submit(raw)
    words.append(eng.fold_words(s0))
    s1 = eng.submit(raw)
    words.append(eng.fold_words(s1))
    eng.wait(s0)
    s2 = eng.submit(raw)
    words.append(eng.fold_words(s2))
    eng.wait(s1)
    eng.wait(s2)
    assert (s0, s1, s2) == (0, 1, 0)
    return eng, words, s2


def test_engine_three_blocks_two_slots(C, raw):
    nbin = 100
    eng, words, slot = run_three(C, raw, nbin)
    assert [w[0] for w in words] == [0, N, 2 * N]
    acc, hits, weights = eng.fold_read()
    wf = eng.waterfall(slot).cpu().numpy()
    want, want_hits, want_w, n_terms = engine_oracle(wf, words, nbin, L)
    assert np.array_equal(hits, want_hits)
    assert np.array_equal(weights, want_w)
    assert_fold_close(acc, want, n_terms)

    # the whole sequence again on a fresh engine: identical bits
    eng2, words2, _ = run_three(C, raw, nbin)
    acc2, hits2, weights2 = eng2.fold_read()
    assert words2 == words
    assert np.array_equal(acc2, acc)
    assert np.array_equal(hits2, hits) and np.array_equal(weights2, weights)

    # reset keeps the stream position
    eng.fold_reset()
    assert eng.fold_next_sample() == 3 * N
    a0, h0, w0 = eng.fold_read()
    assert not a0.any() and not h0.any() and not w0.any()
    slot = eng.submit(raw)
    eng.wait(slot)
    w = eng.fold_words(slot)
    assert w[0] == 3 * N
    acc, hits, weights = eng.fold_read()
    want, want_hits, want_w, n_terms = engine_oracle(wf, [w], nbin, L)
    assert np.array_equal(hits, want_hits)
    assert np.array_equal(weights, want_w)
    assert_fold_close(acc, want, n_terms)


def test_engine_feature_off_is_untouched(C, raw):
    off = make_engine(C)
    on = make_engine(C, **fold_kw(64))
    outs = []
    for eng in (off, on):
        slot = eng.submit(raw)
        res = eng.wait(slot)
        outs.append((res, eng.time_series(slot).cpu().numpy(),
                     eng.waterfall(slot).cpu().numpy()))
    assert outs[0][0] == outs[1][0]
    assert np.array_equal(outs[0][1], outs[1][1])
    assert np.array_equal(outs[0][2], outs[1][2])
    with pytest.raises(RuntimeError):
        off.fold_read()
    with pytest.raises(RuntimeError):
        off.fold_reset()


def test_engine_hip_graph_replays_with_fresh_words(C, raw):
    pinned = raw.pin_memory()
    got = []
    for graph in (False, True):
        eng = make_engine(C, use_hip_graph=graph, **fold_kw(100))
        words = []
        for _ in range(6):
            slot = eng.submit(pinned)
            words.append(eng.fold_words(slot))
            eng.wait(slot)
        got.append((words, eng.fold_read()))
    assert got[0][0] == got[1][0]
    assert len({w[1] for w in got[0][0]}) == 6  # the phases do advance
    for a, b in zip(got[0][1], got[1][1]):
        assert np.array_equal(a, b)
    assert int(got[1][1][1].sum()) == 6 * L


def test_engine_fold_with_filterbank(C, raw):
    fil = dict(fil_tscrunch=16, fil_fscrunch=1, fil_nbits=8)
    both = make_engine(C, **fil, **fold_kw(64))
    only_fil = make_engine(C, **fil)
    only_fold = make_engine(C, **fold_kw(64))
    planes = []
    for eng in (both, only_fil):
        slot = eng.submit(raw)
        eng.wait(slot)
        planes.append(eng.filterbank(slot).numpy().copy())
    slot = only_fold.submit(raw)
    only_fold.wait(slot)
    assert np.array_equal(planes[0], planes[1])
    for a, b in zip(both.fold_read(), only_fold.fold_read()):
        assert np.array_equal(a, b)


@pytest.mark.parametrize("kw,field", [
    (dict(fold_nbin=1, fold_f0=F0), "fold_nbin"),
    (dict(fold_nbin=65537, fold_f0=F0), "fold_nbin"),
    (dict(fold_nbin=64, fold_f0=0.0), "fold_f0"),
    (dict(fold_nbin=64, fold_f0=-1.0), "fold_f0"),
    (dict(fold_nbin=64, fold_f0=RATE / (2 * S)), "fold_f0"),
    (dict(fold_nbin=64, fold_f0=F0, max_dm_trials=2), "max_dm_trials"),
    (dict(fold_nbin=64, fold_f0=F0, nsamps_reserved=2 * S * 3 + 2),
     "nsamps_reserved"),
])
def test_engine_rejections(C, kw, field):
    with pytest.raises(RuntimeError, match=field):
        make_engine(C, **kw)


# ---- 3. both apps on a DM-0 pulse train ----

PERIOD_SAMPLES = 47371.3          # incommensurate with the block, 0.37 ms
PERIOD = PERIOD_SAMPLES / RATE
PULSE_PHASE = 0.3047              # turns: the middle of bin 19 of 64
APP_NBIN = 64
PEAK_BIN = int(PULSE_PHASE * APP_NBIN)

APP_ARGS = [
    "--baseband_input_count", str(N), "--baseband_input_bits", "-8",
    "--spectrum_channel_count", str(S), "--baseband_freq_low", "1400",
    "--baseband_bandwidth", "64", "--baseband_sample_rate", "128e6",
    "--dm", "0",
    "--mitigate_rfi_average_method_threshold", "1e30",
    "--mitigate_rfi_spectral_kurtosis_threshold", "1e30",
    "--signal_detect_signal_noise_threshold", "1e30",
    "--signal_detect_max_boxcar_length", "16",
    "--fold_period", repr(PERIOD), "--fold_nbin", str(APP_NBIN),
    "--fold_subint_blocks", "2",
]


def train_recording(path, n_blocks=4):
    """One-sample pulses (flat across the band) of amplitude 100 at
    (j + PULSE_PHASE) periods in int8 noise of sigma 2, DM 0."""
    n_total = n_blocks * N
    x = np.zeros(n_total)
    j = np.arange(int(n_total / PERIOD_SAMPLES) + 1)
    idx = np.round((j + PULSE_PHASE) * PERIOD_SAMPLES).astype(np.int64)
    x[idx[idx < n_total]] = 100.0
    rng = np.random.default_rng(0)
    np.clip(np.round(x + rng.normal(0, 2, n_total)), -128,
            127).astype(np.int8).view(np.uint8).tofile(path)


def load_subints(stem):
    from srtb_amd.io.writers import fold_subint_paths
    out = []
    for i in range(2):
        p = fold_subint_paths(str(stem), i)
        out.append((np.load(p["profile"]), np.load(p["hits"]),
                    np.load(p["weights"])))
    assert not os.path.exists(fold_subint_paths(str(stem), 2)["profile"])
    return out


@pytest.fixture(scope="module")
def train(tmp_path_factory):
    """The recording and the CPU path's two sub-integrations of it."""
    from srtb_amd.main import main
    d = tmp_path_factory.mktemp("fold_train")
    rec = d / "rec.bin"
    train_recording(rec)
    rc = main(APP_ARGS + [
        "--device", "cpu", "--input_file_path", str(rec),
        "--fold_output_path", str(d / "cpu"),
        "--baseband_output_file_prefix", str(d) + "/c_"])
    assert rc == 0
    return rec, load_subints(d / "cpu")


def check_against_cpu(got, want):
    assert len(got) == len(want) == 2
    for (acc, hits, weights), (c_acc, c_hits, c_weights) in zip(got, want):
        assert acc.dtype == np.float64 and acc.shape == (S, APP_NBIN)
        assert hits.dtype == np.uint64 and weights.dtype == np.uint64
        assert np.array_equal(hits, c_hits)
        assert np.array_equal(weights, c_weights)
        assert int(hits.sum()) == 2 * L
        np.testing.assert_allclose(acc, c_acc, rtol=1e-3,
                                   atol=1e-3 * c_acc.mean())
        peak = int(np.argmax(acc.sum(axis=0) / hits))
        assert abs(peak - PEAK_BIN) <= 1, peak


def test_main_gpu_fold_matches_the_cpu_files(train, tmp_path):
    rec, cpu = train
    from srtb_amd.main import main
    rc = main(APP_ARGS + [
        "--device", "cuda", "--input_file_path", str(rec),
        "--fold_output_path", str(tmp_path / "gpu"),
        "--baseband_output_file_prefix", str(tmp_path) + "/g_"])
    assert rc == 0
    check_against_cpu(load_subints(tmp_path / "gpu"), cpu)


def test_backend_fold_matches_the_cpu_files(train, tmp_path):
    from srtb_amd.io.writers import fold_subint_paths, read_fold_meta
    rec, cpu = train
    r = subprocess.run(
        [BIN, *APP_ARGS, "--input_file_path", str(rec), "--fold_output_path",
         str(tmp_path / "native"), "--baseband_output_file_prefix",
         str(tmp_path) + "/n_"],
        capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    check_against_cpu(load_subints(tmp_path / "native"), cpu)
    for i in range(2):
        meta = read_fold_meta(
            fold_subint_paths(str(tmp_path / "native"), i)["meta"])
        assert int(meta["first_sample"]) == i * 2 * N
        assert int(meta["n_blocks"]) == 2 and int(meta["nbin"]) == APP_NBIN
        assert float(meta["f0"]) == 1.0 / PERIOD
        assert float(meta["tsamp"]) == 2 * S / RATE
