"""GPU tests of the filterbank output: the detect / statistics / quantise
kernels, the engine path that lands every block's rows in pinned host memory,
and srtb-backend writing a .fil file.

Oracle: srtb_amd.ref.filterbank_block / filterbank_quantize in float64, fed
with the GPU's own waterfall (engine tests) or with small-integer waterfalls
whose sums are exact in float32 (stand-alone kernel tests, compared bitwise).
"""

import os
import subprocess

import numpy as np
import pytest
import torch

from srtb_amd import ref
from srtb_amd.config import Config
from srtb_amd.io.writers import filterbank_header, read_filterbank
from srtb_amd.pipeline.cpu import synthesize_dispersed_pulse

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "bin", "srtb-backend")

N, S = 1 << 18, 1 << 6
L = N // 2 // S
ZAP = [[100, 300]]
TONE_ROW = 20  # waterfall row the sweeping tone sits in


@pytest.fixture(scope="module")
def C():
    from srtb_amd.ops import native
    torch.cuda.set_device(0)
    return native()


def make_engine(C, bandwidth=64.0, fft=0, **kw):
    args = dict(
        n=N, nbits=-8, channels=S,
        freq_low=1400.0 if bandwidth > 0 else 1464.0, bandwidth=bandwidth,
        sample_rate=128e6, dm=60.0, rfi_threshold=20.0, sk_threshold=1.5,
        snr_threshold=6.0, max_boxcar=16, nsamps_reserved=0, zap_ranges=ZAP,
        use_phase_table=False, enable_rfi_s1=True, enable_sk=True, n_slots=2,
        fft_backend=fft)
    args.update(kw)
    return C.PipelineEngine(**args)


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
    cfg.baseband_sample_rate = 128e6
    cfg.dm = 60.0
    raw = synthesize_dispersed_pulse(
        cfg, 0.3 * N / 128e6, pulse_amp=7.5, noise_sigma=16.0,
        rng=np.random.default_rng(seed), width=1)
    t = np.arange(N, dtype=np.float64)
    f0, f1 = TONE_ROW * 1e6 / 128e6, (TONE_ROW + 1) * 1e6 / 128e6
    tone = 10.0 * np.cos(2 * np.pi * (f0 * t + 0.5 * (f1 - f0) * t * t / N))
    x = raw.view(np.int8).astype(np.float64) + np.round(tone)
    return torch.from_numpy(
        np.clip(x, -128, 127).astype(np.int8).view(np.uint8).copy())


@pytest.fixture(scope="module")
def raw():
    return make_block()


def oracle_plane(eng, slot, valid, tscrunch, fscrunch, reverse):
    """fp64 oracle from the GPU's own (zapped) waterfall."""
    wf = eng.waterfall(slot).cpu().numpy()
    return ref.filterbank_block(wf, valid, tscrunch, fscrunch, reverse)


# ---- 1. power plane against the oracle ----

@pytest.mark.parametrize("odd_rows", [False, True])
@pytest.mark.parametrize("fft", [0, 1])
@pytest.mark.parametrize("bandwidth", [64.0, -64.0])
@pytest.mark.parametrize("tscrunch,fscrunch",
                         [(1, 1), (2, 4), (16, 1), (1, 64), (64, 64)])
def test_power_plane_matches_oracle(C, raw, tscrunch, fscrunch, bandwidth,
                                    fft, odd_rows):
    reserved = 2 * S * tscrunch * 3 if odd_rows else 0
    eng = make_engine(C, bandwidth=bandwidth, fft=fft,
                      nsamps_reserved=reserved, fil_tscrunch=tscrunch,
                      fil_fscrunch=fscrunch, fil_nbits=32)
    valid = (N - reserved) // (2 * S)
    R, Cn = valid // tscrunch, S // fscrunch
    assert (eng.filterbank_rows, eng.filterbank_channels) == (R, Cn)
    if odd_rows:
        assert R % 2 == 1
        assert valid != eng.ts_count  # ts_count drops twice as much
    slot = eng.submit(raw)
    res = eng.wait(slot)
    assert res["zero_count"] > 0  # at least the tone's row is flagged
    host = eng.filterbank(slot)
    got = eng.filterbank_power(slot).cpu().numpy()
    assert host.dtype == torch.float32 and tuple(host.shape) == (R, Cn)
    assert np.array_equal(host.numpy(), got)
    # read after the filterbank: this applies the deferred zap
    want = oracle_plane(eng, slot, valid, tscrunch, fscrunch, bandwidth > 0)
    rtol = (tscrunch * fscrunch + 2) * 2.0 ** -23
    err = np.abs(got - want) / np.where(want > 0, want, 1.0)
    print("max rel err", err.max(), "bound", rtol)
    np.testing.assert_allclose(got, want, rtol=rtol, atol=0)
    assert (want > 0).any()
    if fscrunch == 1:
        c = S - 1 - TONE_ROW if bandwidth > 0 else TONE_ROW
        assert (want[:, c] == 0).all()
        assert (got[:, c] == 0).all()


# ---- 2. stand-alone kernel on shapes the engine cannot make ----

def distinct_waterfall(S_, L_):
    """Every element distinct, small integers: re = t - 40, im = row - 90."""
    re = np.arange(L_, dtype=np.float64)[None, :] - 40.0
    im = np.arange(S_, dtype=np.float64)[:, None] - 90.0
    return (re + 1j * im).astype(np.complex64)


def pattern_waterfall(S_, L_):
    """Small integers without symmetry in row or time, |.|^2 <= 421."""
    t = np.arange(L_)[None, :]
    r = np.arange(S_)[:, None]
    re = (t * 7 + r * 3) % 31 - 15
    im = (t * 5 + r * 11) % 29 - 14
    return (re + 1j * im).astype(np.complex64)


KERNEL_CASES = [
    # fill, S, L, V, tscrunch, fscrunch
    ("distinct", 6, 10, 6, 1, 1),
    ("distinct", 6, 10, 6, 2, 3),
    ("distinct", 6, 10, 6, 2, 6),        # C = 1
    ("distinct", 192, 96, 72, 8, 64),    # R = 9, C = 3, V < L
    ("pattern", 70, 300, 149, 1, 1),     # odd V: the last float4 straddles it
    ("pattern", 70, 300, 150, 2, 1),     # R = 75, C = 70: partial tiles
    ("pattern", 66, 200, 200, 4, 2),     # C = 33: one channel past a tile
    ("pattern", 5, 4096, 4000, 32, 5),   # 16 lanes per cell, R = 125, C = 1
    ("pattern", 3, 2048, 1536, 256, 1),  # 64 lanes per cell, 2 loads per lane
    ("pattern", 2, 8192, 8192, 4096, 2),  # the largest tscrunch
]


@pytest.mark.parametrize("with_flags", [False, True])
@pytest.mark.parametrize("reverse", [False, True])
@pytest.mark.parametrize("fill,S_,L_,V,tscrunch,fscrunch", KERNEL_CASES)
def test_detect_kernel_exact(C, fill, S_, L_, V, tscrunch, fscrunch, reverse,
                             with_flags):
    wf = (distinct_waterfall if fill == "distinct" else pattern_waterfall)(
        S_, L_)
    flags = None
    zapped = wf.copy()
    if with_flags:
        f = np.zeros(S_, dtype=np.uint8)
        f[[0, S_ // 2, S_ - 1]] = 1
        zapped[f != 0] = 0
        flags = torch.from_numpy(f).cuda()
    want = ref.filterbank_block(zapped, V, tscrunch, fscrunch, reverse)
    assert want.max() < 2 ** 24  # every partial sum is exact in float32
    got = C.filterbank_detect(torch.from_numpy(wf).cuda(), flags, V, tscrunch,
                              fscrunch, reverse).cpu().numpy()
    assert got.shape == (V // tscrunch, S_ // fscrunch)
    assert got.dtype == np.float32
    assert np.array_equal(got, want.astype(np.float32)), \
        np.argwhere(got != want.astype(np.float32))[:8]


def test_detect_kernel_rejects_bad_geometry(C):
    wf = torch.zeros(6, 10, dtype=torch.complex64).cuda()
    for args in [(6, 1, 4, False), (11, 1, 1, False), (1, 2, 1, False)]:
        with pytest.raises(RuntimeError):
            C.filterbank_detect(wf, None, *args)
    with pytest.raises(RuntimeError):  # not a power of two
        C.filterbank_detect(wf, None, 6, 3, 1, False)
    with pytest.raises(RuntimeError):  # odd row length
        C.filterbank_detect(torch.zeros(6, 9, dtype=torch.complex64).cuda(),
                            None, 6, 1, 1, False)


# ---- 3. statistics ----

@pytest.fixture(scope="module")
def eight_bit(C, raw):
    """One 8-bit block: engine, slot, result."""
    eng = make_engine(C, fil_tscrunch=2, fil_fscrunch=1, fil_nbits=8)
    slot = eng.submit(raw)
    res = eng.wait(slot)
    return eng, slot, res


def test_channel_stats_match_numpy(C, eight_bit):
    eng, slot, res = eight_bit
    assert res["zero_count"] > 0
    P = eng.filterbank_power(slot).cpu().numpy().astype(np.float64)
    mean, std = (t.numpy() for t in eng.filterbank_stats(slot))
    assert mean.dtype == std.dtype == np.float32
    assert mean.shape == std.shape == (S,)
    np.testing.assert_allclose(mean, P.mean(axis=0), rtol=1e-6, atol=0)
    np.testing.assert_allclose(std, P.std(axis=0), rtol=1e-6, atol=0)
    c = S - 1 - TONE_ROW
    assert mean[c] == 0 and std[c] == 0
    assert (eng.filterbank(slot).numpy()[:, c] == 64).all()
    # the module-level kernel gives the same floats
    m2, s2 = C.filterbank_channel_stats(eng.filterbank_power(slot))
    assert np.array_equal(m2.cpu().numpy(), mean)
    assert np.array_equal(s2.cpu().numpy(), std)


@pytest.mark.parametrize("R,Cn", [(1, 1), (3, 5), (63, 65), (1000, 7)])
def test_channel_stats_kernel_shapes(C, R, Cn):
    rng = np.random.default_rng(R * 100 + Cn)
    P = rng.gamma(4.0, 3.0, (R, Cn)).astype(np.float32)
    P[:, 0] = 7.25  # a constant channel has exactly zero deviation
    mean, std = C.filterbank_channel_stats(torch.from_numpy(P).cuda())
    P64 = P.astype(np.float64)
    np.testing.assert_allclose(mean.cpu().numpy(), P64.mean(axis=0),
                               rtol=1e-6, atol=0)
    np.testing.assert_allclose(std.cpu().numpy(), P64.std(axis=0), rtol=1e-6,
                               atol=0)
    assert float(std[0]) == 0.0 and float(mean[0]) == 7.25


# ---- 4. quantisation ----

def check_quantised(q, P, mean, std):
    want = ref.filterbank_quantize(P.astype(np.float64), mean, std)
    diff = np.abs(q.astype(np.int32) - want.astype(np.int32))
    print("levels off by one:", int((diff > 0).sum()), "of", diff.size)
    assert diff.max() <= 1
    assert (diff > 0).mean() <= 1e-3


def test_quantised_plane_matches_oracle(C, eight_bit):
    eng, slot, _ = eight_bit
    q = eng.filterbank(slot)
    assert q.dtype == torch.uint8
    assert tuple(q.shape) == (eng.filterbank_rows, eng.filterbank_channels)
    q = q.numpy()
    P = eng.filterbank_power(slot).cpu().numpy()
    mean, std = (t.numpy() for t in eng.filterbank_stats(slot))
    check_quantised(q, P, mean, std)
    assert (q == 255).any()  # the pulse saturates
    live = np.delete(q, S - 1 - TONE_ROW, axis=1)
    assert np.abs(live.astype(np.float64).mean(axis=0) - 64).max() < 1.0


@pytest.mark.parametrize("R,Cn", [(1, 1), (3, 5), (63, 65), (257, 3)])
def test_quantize_kernel_shapes(C, R, Cn):
    """R * Cn not a multiple of 4, C not a multiple of 4: the packed stores and
    the scalar tail both index the right channel."""
    rng = np.random.default_rng(R * 100 + Cn)
    P = rng.gamma(4.0, 3.0, (R, Cn)).astype(np.float32)
    mean = (12.0 + np.arange(Cn)).astype(np.float32)
    std = (1.0 + 0.5 * np.arange(Cn)).astype(np.float32)
    std[Cn // 2] = 0.0
    q = C.filterbank_quantize(torch.from_numpy(P).cuda(),
                              torch.from_numpy(mean).cuda(),
                              torch.from_numpy(std).cuda()).cpu().numpy()
    assert q.shape == (R, Cn) and q.dtype == np.uint8
    want = ref.filterbank_quantize(P, mean, std)
    assert np.abs(q.astype(np.int32) - want.astype(np.int32)).max() <= 1
    assert (q != want).sum() <= max(1, q.size // 1000)
    assert (q[:, Cn // 2] == 64).all()


# ---- 5. determinism and isolation ----

@pytest.mark.parametrize("nbits", [8, 32])
def test_both_slots_give_identical_planes(C, raw, nbits):
    eng = make_engine(C, fil_tscrunch=16, fil_fscrunch=2, fil_nbits=nbits)
    slots = [eng.submit(raw), eng.submit(raw)]
    assert slots == [0, 1]
    planes = []
    for slot in slots:
        eng.wait(slot)
        planes.append((eng.filterbank(slot).clone(),
                       eng.filterbank_power(slot).clone()))
    assert torch.equal(planes[0][0], planes[1][0])
    assert torch.equal(planes[0][1], planes[1][1])
    # and again on the first slot
    slot = eng.submit(raw)
    assert slot == 0
    eng.wait(slot)
    assert torch.equal(eng.filterbank(slot), planes[0][0])
    assert torch.equal(eng.filterbank_power(slot), planes[0][1])


@pytest.mark.parametrize("fft", [0, 1])
def test_feature_leaves_the_chain_unchanged(C, raw, fft):
    off = make_engine(C, fft=fft)
    on = make_engine(C, fft=fft, fil_tscrunch=16, fil_fscrunch=1, fil_nbits=8)
    assert (off.filterbank_rows, off.filterbank_channels) == (0, 0)
    with pytest.raises(RuntimeError):
        off.filterbank(0)
    so, sn = off.submit(raw), on.submit(raw)
    ro, rn = off.wait(so), on.wait(sn)
    assert ro == rn
    assert torch.equal(off.time_series(so), on.time_series(sn))
    assert torch.equal(torch.view_as_real(off.waterfall(so)),
                       torch.view_as_real(on.waterfall(sn)))


def test_hip_graph_replay_gives_the_same_plane(C, raw):
    pinned = raw.clone().pin_memory()
    eng = make_engine(C, use_hip_graph=True, fil_tscrunch=16, fil_fscrunch=1,
                      fil_nbits=8)
    first = None
    # per slot: direct, captured, then replayed submissions
    for i in range(6):
        slot = eng.submit(pinned)
        res = eng.wait(slot)
        plane = eng.filterbank(slot).clone()
        power = eng.filterbank_power(slot).clone()
        if first is None:
            first = (res, plane, power)
        assert res == first[0], i
        assert torch.equal(plane, first[1]), i
        assert torch.equal(power, first[2]), i


# ---- 6. rejections ----

@pytest.mark.parametrize("kw,match", [
    (dict(fil_tscrunch=12), "fil_tscrunch"),
    (dict(fil_tscrunch=8192), "fil_tscrunch"),
    (dict(fil_tscrunch=4, fil_fscrunch=3), "fil_fscrunch"),
    (dict(fil_tscrunch=4, fil_fscrunch=128), "fil_fscrunch"),
    (dict(fil_tscrunch=16, nsamps_reserved=2 * S * 8), "multiple"),
    (dict(fil_tscrunch=4, fil_nbits=16), "fil_nbits"),
    (dict(fil_tscrunch=4, max_dm_trials=2), "max_dm_trials"),
])
def test_constructor_rejections(C, kw, match):
    with pytest.raises(RuntimeError, match=match):
        make_engine(C, **kw)


def test_phase_table_stays_allowed(C, raw):
    eng = make_engine(C, use_phase_table=True, fil_tscrunch=4, fil_nbits=32)
    slot = eng.submit(raw)
    eng.wait(slot)
    got = eng.filterbank_power(slot).cpu().numpy()
    want = oracle_plane(eng, slot, L, 4, 1, True)
    np.testing.assert_allclose(got, want, rtol=6 * 2.0 ** -23, atol=0)


# ---- 7. native app ----

@pytest.mark.skipif(not os.path.exists(BIN), reason="native binaries not built")
def test_srtb_backend_writes_filterbank(tmp_path):
    """noise, pulse, noise through srtb-backend, 8-bit, tscrunch 4."""
    tscrunch = 4
    cfg = Config()
    cfg.baseband_input_count = N
    cfg.spectrum_channel_count = S
    cfg.baseband_input_bits = -8
    cfg.baseband_freq_low = 1400.0
    cfg.baseband_bandwidth = 64.0
    cfg.baseband_sample_rate = 128e6
    cfg.dm = 60.0
    rng = np.random.default_rng(0)
    noise = [np.clip(np.round(rng.normal(0, 2, N)), -128,
                     127).astype(np.int8).view(np.uint8) for _ in range(2)]
    pulse_index = int(0.4 * N)
    pulse = synthesize_dispersed_pulse(cfg, pulse_index / 128e6,
                                       pulse_amp=40.0, noise_sigma=2.0,
                                       width=1)
    rec = tmp_path / "rec.bin"
    np.concatenate([noise[0], pulse, noise[1]]).tofile(rec)
    fil = tmp_path / "out.fil"

    out = subprocess.run(
        ["timeout", "-k", "10", "240", BIN, "--input_file_path", str(rec),
         "--baseband_input_count", str(N), "--baseband_input_bits", "-8",
         "--spectrum_channel_count", str(S),
         "--baseband_freq_low", "1400", "--baseband_bandwidth", "64",
         "--baseband_sample_rate", "128e6", "--dm", "60",
         "--mitigate_rfi_average_method_threshold", "1e30",
         "--mitigate_rfi_spectral_kurtosis_threshold", "1e30",
         "--signal_detect_signal_noise_threshold", "6",
         "--signal_detect_max_boxcar_length", "16",
         "--filterbank_output_path", str(fil),
         "--filterbank_tscrunch", str(tscrunch), "--filterbank_nbits", "8",
         "--filterbank_tstart_mjd", "60000.5",
         "--baseband_output_file_prefix", str(tmp_path) + "/out_"],
        capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr
    assert "blocks=3" in out.stdout, (out.stdout, out.stderr)

    kw = ref.filterbank_header_fields(1400.0, 64.0, 128e6, S, tscrunch, 1)
    kw.update(nbits=8, tstart=60000.5)
    header = filterbank_header(**kw)
    blob = fil.read_bytes()
    assert blob[:len(header)] == header
    R = N // (2 * S * tscrunch)
    assert len(blob) == len(header) + 3 * R * S
    _, data = read_filterbank(str(fil))
    assert data.shape == (3 * R, S) and data.dtype == np.uint8
    row = int(np.argmax(data.astype(np.float64).sum(axis=1)))
    want = (N + pulse_index) // (2 * S * tscrunch)
    assert abs(row - want) <= 1, (row, want)
    assert (data[row] == 255).sum() >= 0.75 * S


# ---- 8. srtb_amd.main on the GPU ----

def test_main_gpu_file_matches_the_cpu_file(tmp_path):
    """The same recording through the GPU engine and through the oracle path
    gives the same header and, up to the float32 transforms, the same plane."""
    from srtb_amd.main import main
    from tests.test_filterbank_cpu import (APP_ARGS, check_pulse_file,
                                           pulse_recording)
    rec = tmp_path / "rec.bin"
    pulse_recording(rec)
    files = {}
    for dev in ("cuda", "cpu"):
        out = tmp_path / f"{dev}.fil"
        rc = main(APP_ARGS + [
            "--device", dev, "--input_file_path", str(rec),
            "--filterbank_output_path", str(out), "--filterbank_nbits", "32",
            "--baseband_output_file_prefix", f"{tmp_path}/{dev}_"])
        assert rc == 0
        check_pulse_file(out, 32)
        files[dev] = out
    hg, gpu = read_filterbank(str(files["cuda"]))
    hc, cpu = read_filterbank(str(files["cpu"]))
    assert hg == hc
    # fp32 transforms of 2^17 points: errors ~1e-5 of the mean power per
    # cell; 1e-3 of the mean is a 100-fold margin
    np.testing.assert_allclose(gpu, cpu, rtol=1e-3,
                               atol=1e-3 * float(cpu.mean()))


def test_main_gpu_two_pol_writes_one_file_per_stream(tmp_path):
    from srtb_amd.main import main
    from tests.test_filterbank_cpu import TWO_POL_ARGS, check_two_pol_files
    from tests.test_main_app import make_2pol_recording
    _, rec = make_2pol_recording(tmp_path)
    rc = main(TWO_POL_ARGS + [
        "--input_file_path", rec,
        "--filterbank_output_path", str(tmp_path / "pol.fil"),
        "--baseband_output_file_prefix", str(tmp_path) + "/p2_"])
    assert rc == 0
    check_two_pol_files(tmp_path)
