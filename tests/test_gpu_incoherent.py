"""GPU tests of the incoherent DM-offset search: the dedisperse and detect
kernels, the streaming IncoherentSearch object and the engine end to end.

Oracle: srtb_amd.ref.incoherent_* in float64.  The kernel tests use small
integers, for which every float32 sum (dedisperse) and every float64 mean,
scan and sum of squares (detect) is exact, and compare bit for bit.
"""

import numpy as np
import pytest
import torch

from srtb_amd import ref
from srtb_amd.config import Config
from srtb_amd.pipeline.cpu import synthesize_dispersed_pulse

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def C():
    from srtb_amd.ops import native
    torch.cuda.set_device(0)
    return native()


def gpu_dedisperse(C, window, delays, R):
    return C.incoh_dedisperse(
        torch.from_numpy(np.ascontiguousarray(window, dtype=np.float32)).cuda(),
        torch.from_numpy(np.ascontiguousarray(delays, dtype=np.int32)).cuda(),
        R).cpu().numpy()


# ---- 1. dedisperse ----

def test_dedisperse_exact_on_the_shape_grid(C):
    """Small-integer planes, random non-monotone tables in 0..D_max."""
    chunk = C.INCOH_CHANNEL_CHUNK
    rng = np.random.default_rng(1)
    cases = 0
    for Cn in (1, 3, 64, 65, chunk + 1):
        for R in (2, 8, 96, 128):
            for D in (0, 1, R - 1, R, 2 * R + 3):
                window = rng.integers(-7, 8, (D + R, Cn)).astype(np.float32)
                for T in (1, 5, 64):
                    delays = rng.integers(0, D + 1, (T, Cn)).astype(np.int32)
                    delays[0, 0], delays[-1, -1] = D, 0  # both ends are used
                    want = ref.incoherent_dedisperse(window, delays, R)
                    assert np.abs(want).max() < 2 ** 24
                    got = gpu_dedisperse(C, window, delays, R)
                    assert got.shape == (T, R) and got.dtype == np.float32
                    assert np.array_equal(got, want.astype(np.float32)), \
                        (Cn, R, D, T, np.argwhere(got != want)[:4])
                    cases += 1
    assert cases == 5 * 4 * 5 * 3


def test_dedisperse_real_values_within_the_summation_bound(C):
    """|Y - Y64| <= C * 2^-24 * sum_c |X| over the gathered terms: the
    worst-case float32 summation bound of any order."""
    rng = np.random.default_rng(2)
    chunk = C.INCOH_CHANNEL_CHUNK
    for Cn, R, D, T in [(65, 96, 40, 5), (2 * chunk + 77, 33, 9, 7)]:
        window = rng.normal(10.0, 4.0, (D + R, Cn)).astype(np.float32)
        delays = rng.integers(0, D + 1, (T, Cn)).astype(np.int32)
        want = ref.incoherent_dedisperse(window, delays, R)
        bound = Cn * 2.0 ** -24 * ref.incoherent_dedisperse(
            np.abs(window), delays, R)
        got = gpu_dedisperse(C, window, delays, R)
        err = np.abs(got.astype(np.float64) - want)
        print("max err / bound", (err / bound).max())
        assert (err <= bound).all()


def test_dedisperse_is_deterministic(C):
    rng = np.random.default_rng(3)
    Cn, R, D, T = 2 * C.INCOH_CHANNEL_CHUNK + 5, 40, 17, 6
    window = rng.normal(0, 1, (D + R, Cn)).astype(np.float32)
    delays = rng.integers(0, D + 1, (T, Cn)).astype(np.int32)
    first = gpu_dedisperse(C, window, delays, R)
    for _ in range(3):
        assert np.array_equal(gpu_dedisperse(C, window, delays, R), first)


# ---- 2. detect ----

def ulp_close(a, b, ulps):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return np.abs(a - b) <= ulps * np.spacing(np.maximum(np.abs(a), np.abs(b)))


def check_clear_of_thresholds(Y, snr, max_boxcar, rel):
    """No oracle boxcar value within `rel` (relative) of its threshold: a
    condition on the input that makes the counts well-defined."""
    for y in np.asarray(Y, dtype=np.float64):
        for l in ref.incoherent_lengths(max_boxcar):
            _, b = ref.incoherent_series(y, l)
            if b.size == 0:
                continue
            thr = snr * np.sqrt((b * b).sum() / b.size)
            assert (np.abs(b - thr) > rel * abs(thr)).all() or thr == 0


def run_detect(C, Y, snr, max_boxcar):
    out = C.incoh_detect(torch.from_numpy(Y.astype(np.float32)).cuda(), snr,
                         max_boxcar)
    return [o.cpu().numpy() for o in out]


@pytest.mark.parametrize("R,max_boxcar,seed", [(8, 4, 11), (128, 16, 12)])
def test_detect_exact_on_small_integers(C, R, max_boxcar, seed):
    rng = np.random.default_rng(seed)
    T, snr = 9, 1.5
    Y = rng.integers(-1023, 1024, (T, R)).astype(np.float64)
    Y[1] = rng.integers(-2, 3, R)  # many ties, peaks included
    Y[2] = 0
    Y[2, [R // 4, R // 2, R - 1]] = 5  # the same peak three times
    check_clear_of_thresholds(Y, snr, max_boxcar, 8 * 2.0 ** -52)
    want = ref.incoherent_detect(Y, snr, max_boxcar)
    peak, index, rms, count, mu = run_detect(C, Y, snr, max_boxcar)
    assert np.array_equal(mu, want["mu"])
    assert np.array_equal(peak, want["peak"])
    assert np.array_equal(index, want["index"])
    assert ulp_close(rms, want["rms"], 4).all()
    assert ulp_close(snr * rms, snr * want["rms"], 4).all()
    assert np.array_equal(count, want["count"])
    assert (want["count"] > 1).any()
    assert want["index"][2, 0] == R // 4


def test_detect_rows_not_a_power_of_two(C):
    rng = np.random.default_rng(13)
    T, R, snr, max_boxcar = 6, 96, 2.0, 32
    Y = rng.normal(100.0, 10.0, (T, R)).astype(np.float32).astype(np.float64)
    check_clear_of_thresholds(Y, snr, max_boxcar, 2.0 ** -36)
    want = ref.incoherent_detect(Y, snr, max_boxcar)
    peak, index, rms, count, mu = run_detect(C, Y, snr, max_boxcar)
    # neither the mean nor the scan is exact here: relative 2^-40
    for got, exp in ((mu, want["mu"]), (peak, want["peak"]),
                     (rms, want["rms"])):
        assert (exp > 0).all()
        assert (np.abs(got - exp) <= 2.0 ** -40 * exp).all()
    assert np.array_equal(index, want["index"])
    assert np.array_equal(count, want["count"])


def test_detect_lengths_without_a_window_and_a_constant_row(C):
    T, R, max_boxcar = 3, 8, 32
    Y = np.array([[3, 1, 4, 1, 5, 9, 2, 6], [7] * 8, [0, 0, 0, 0, 0, 0, 0, 8]],
                 dtype=np.float64)
    want = ref.incoherent_detect(Y, 1.0, max_boxcar)
    peak, index, rms, count, mu = run_detect(C, Y, 1.0, max_boxcar)
    assert peak.shape == (T, 6)  # 1, 2, 4, 8, 16, 32
    assert np.isneginf(peak[:, 3:]).all() and (index[:, 3:] == -1).all()
    assert (rms[:, 3:] == 0).all() and (count[:, 3:] == 0).all()
    assert (rms[1] == 0).all() and (count[1] == 0).all()
    assert (peak[1, :3] == 0).all() and (index[1, :3] == 0).all()
    assert np.array_equal(peak, want["peak"])
    assert np.array_equal(index, want["index"])
    assert np.array_equal(count, want["count"])
    assert np.array_equal(mu, want["mu"])
    assert ulp_close(rms, want["rms"], 4).all()


def test_detect_at_the_largest_row_count(C):
    """R = 16384 fills the workgroup's LDS.  Integer rows that sum to zero:
    mu = 0, so z, the scan and the sums of squares are exact integers."""
    rng = np.random.default_rng(14)
    R = C.INCOH_MAX_ROWS
    Y = rng.integers(-8, 9, (2, R)).astype(np.float64)
    Y[:, -1] -= Y.sum(axis=1)
    assert (Y.sum(axis=1) == 0).all() and np.abs(Y).max() < 2 ** 20
    want = ref.incoherent_detect(Y, 3.0, 64)
    peak, index, rms, count, mu = run_detect(C, Y, 3.0, 64)
    assert (mu == 0).all()
    assert np.array_equal(peak, want["peak"])
    assert np.array_equal(index, want["index"])
    assert ulp_close(rms, want["rms"], 4).all()
    # counts: thresholds differ by a few ulp at most and the values are
    # integers, so only an integer threshold could split them
    assert (np.floor(3.0 * want["rms"]) != 3.0 * want["rms"]).all()
    assert np.array_equal(count, want["count"])


# ---- 3. streaming ----

STREAM = dict(R=8, C=16, fch1=1463.5, foff=-4.0, tsamp=2.5e-4,
              offsets=[-30.0, 0.0, 12.5, 40.0], snr_threshold=2.0,
              max_boxcar=4)


def same_result(got, want):
    assert got["valid"] == want["valid"]
    assert got["first_row"] == want["first_row"]
    assert got["block"] == want["block"]
    assert len(got["trials"]) == len(want["trials"])
    for g, w in zip(got["trials"], want["trials"]):
        assert g["offset"] == w["offset"] and g["mean"] == w["mean"]
        for gl, wl in zip(g["lengths"], w["lengths"]):
            for key in ("boxcar_length", "peak", "index", "count"):
                assert gl[key] == wl[key], (key, gl, wl)
            assert ulp_close(gl["rms"], wl["rms"], 4)
            assert ulp_close(gl["snr"], wl["snr"], 8)


def test_streaming_matches_the_cpu_search(C):
    kw = dict(STREAM)
    R, Cn = kw.pop("R"), kw.pop("C")
    gpu = C.IncoherentSearch(rows=R, channels=Cn, **kw)
    cpu = ref.CpuIncoherentSearch(R, Cn, **kw)
    assert np.array_equal(gpu.delays().numpy(), cpu.delays)
    assert gpu.d_max == cpu.d_max and cpu.d_max > 2 * R
    rng = np.random.default_rng(4)
    planes = [rng.integers(0, 16, (R, Cn)).astype(np.float32)
              for _ in range(6)]
    dev = [torch.from_numpy(p).cuda() for p in planes]

    def run(ps):
        # two in flight, as the engine's two slots
        out, pending = [], []
        for p in ps:
            pending.append(gpu.submit_plane(p))
            if len(pending) == 2:
                k = pending.pop(0)
                out.append((gpu.wait(k), gpu.plane(k).numpy()))
        for k in pending:
            out.append((gpu.wait(k), gpu.plane(k).numpy()))
        return out

    valid = []
    for (res, Y), p in zip(run(dev), planes):
        want = cpu.add(p)
        same_result(res, want)
        assert np.array_equal(Y, want["Y"].astype(np.float32))
        valid.append(res["valid"])
    first_valid = -(-cpu.d_max // R)
    assert valid == [b >= first_valid for b in range(6)] and any(valid)

    gpu.reset()
    cpu.reset()
    for (res, Y), p in zip(run(dev[3:]), planes[3:]):
        want = cpu.add(p)
        same_result(res, want)
        assert np.array_equal(Y, want["Y"].astype(np.float32))
    assert res["block"] == 2 and not res["valid"]


# ---- 4. engine end to end ----

N, S, TSCRUNCH = 1 << 18, 1 << 6, 16


def make_engine(C, **kw):
    args = dict(
        n=N, nbits=-8, channels=S, freq_low=1400.0, bandwidth=64.0,
        sample_rate=128e6, dm=60.0, rfi_threshold=1e30, sk_threshold=1e30,
        snr_threshold=6.0, max_boxcar=16, nsamps_reserved=0, zap_ranges=[],
        use_phase_table=False, enable_rfi_s1=True, enable_sk=True, n_slots=2,
        fil_tscrunch=TSCRUNCH, fil_fscrunch=1, fil_nbits=32)
    args.update(kw)
    return C.PipelineEngine(**args)


PULSE_INDEX = int(0.4 * N)


@pytest.fixture(scope="module")
def blocks():
    """noise, a pulse at DM 62, noise"""
    cfg = Config()
    cfg.baseband_input_count = N
    cfg.spectrum_channel_count = S
    cfg.baseband_input_bits = -8
    cfg.baseband_freq_low = 1400.0
    cfg.baseband_bandwidth = 64.0
    cfg.baseband_sample_rate = 128e6
    cfg.dm = 62.0
    rng = np.random.default_rng(0)
    noise = [np.clip(np.round(rng.normal(0, 2, N)), -128,
                     127).astype(np.int8).view(np.uint8) for _ in range(2)]
    pulse = synthesize_dispersed_pulse(cfg, PULSE_INDEX / 128e6,
                                       pulse_amp=40.0, noise_sigma=2.0,
                                       width=1)
    return [torch.from_numpy(b.copy()) for b in (noise[0], pulse, noise[1])]


def search_args(offsets):
    hdr = ref.filterbank_header_fields(1400.0, 64.0, 128e6, S, TSCRUNCH, 1)
    return dict(fch1=hdr["fch1"], foff=hdr["foff"], tsamp=hdr["tsamp"],
                offsets=offsets, snr_threshold=6.0, max_boxcar=16)


def best_snr(trial):
    return max(l["snr"] for l in trial["lengths"])


def test_engine_end_to_end_recovers_the_offset(C, blocks):
    offsets = [float(x) for x in range(-2, 5)]
    eng = make_engine(C)
    R, Cn = eng.filterbank_rows, eng.filterbank_channels
    assert (R, Cn) == (N // (2 * S * TSCRUNCH), S)
    kw = search_args(offsets)
    gpu = C.IncoherentSearch(rows=R, channels=Cn, **kw)
    cpu = ref.CpuIncoherentSearch(R, Cn, **kw)
    assert 0 < gpu.d_max < R
    results = []
    for raw in blocks:
        slot = eng.submit(raw)
        k = gpu.submit(eng, slot)  # without waiting for the engine
        eng.wait(slot)
        res = gpu.wait(k)
        plane = eng.filterbank_power(slot).cpu().numpy()
        want = cpu.add(plane)
        Y = gpu.plane(k).numpy()
        bound = Cn * 2.0 ** -24 * ref.incoherent_dedisperse(
            np.abs(cpu.window), cpu.delays, R)
        assert (np.abs(Y - want["Y"]) <= bound).all()
        assert res["valid"] == want["valid"]
        assert res["first_row"] == want["first_row"]
        results.append((res, want))
    assert [r["valid"] for r, _ in results] == [False, True, True]

    # the pulse's row: block 1 or 2, whichever holds the higher snr
    res, want = max((rw for rw in results if rw[0]["valid"]),
                    key=lambda rw: max(best_snr(t) for t in rw[0]["trials"]))
    snrs = [best_snr(t) for t in res["trials"]]
    print("best snr per offset", dict(zip(offsets, snrs)))
    best = int(np.argmax(snrs))
    assert offsets[best] == 2.0
    assert snrs[best] > snrs[offsets.index(0.0)]
    top = max(res["trials"][best]["lengths"], key=lambda l: l["snr"])
    wtop = max(want["trials"][best]["lengths"], key=lambda l: l["snr"])
    assert top["boxcar_length"] == wtop["boxcar_length"]
    assert top["index"] == wtop["index"]
    row = res["first_row"] + top["index"]
    expect = (N + PULSE_INDEX) // (2 * S * TSCRUNCH)
    assert abs(row - expect) <= top["boxcar_length"] + 1, (row, expect)


def test_zero_offset_is_the_channel_sum(C, blocks):
    eng = make_engine(C)
    R, Cn = eng.filterbank_rows, eng.filterbank_channels
    gpu = C.IncoherentSearch(rows=R, channels=Cn, **search_args([0.0]))
    assert gpu.d_max == 0
    slot = eng.submit(blocks[1])
    k = gpu.submit(eng, slot)
    eng.wait(slot)
    res = gpu.wait(k)
    assert res["valid"] and res["first_row"] == 0
    plane = eng.filterbank_power(slot).cpu().numpy().astype(np.float64)
    want = plane.sum(axis=1)
    bound = Cn * 2.0 ** -24 * np.abs(plane).sum(axis=1)
    assert (np.abs(gpu.plane(k).numpy()[0] - want) <= bound).all()


def test_submit_rejects_another_geometry(C):
    eng = make_engine(C)
    gpu = C.IncoherentSearch(rows=eng.filterbank_rows // 2,
                             channels=eng.filterbank_channels,
                             **search_args([0.0]))
    with pytest.raises(RuntimeError, match="filterbank plane"):
        gpu.submit(eng, 0)


# ---- 5. argument rejection, before any launch ----

def test_kernel_bindings_reject_bad_arguments(C):
    f32 = lambda *s: torch.zeros(*s, dtype=torch.float32).cuda()  # noqa: E731
    i32 = lambda *s: torch.zeros(*s, dtype=torch.int32).cuda()  # noqa: E731
    with pytest.raises(RuntimeError, match="trials"):  # T = 0
        C.incoh_dedisperse(f32(12, 4), i32(0, 4), 8)
    with pytest.raises(RuntimeError, match="R must be"):  # R = 1
        C.incoh_dedisperse(f32(12, 4), i32(2, 4), 1)
    with pytest.raises(RuntimeError, match="R must be"):  # R > window
        C.incoh_dedisperse(f32(12, 4), i32(2, 4), 13)
    for bad in (5, -1):  # D_max = 4
        d = i32(2, 4)
        d[1, 2] = bad
        with pytest.raises(RuntimeError, match="delays must lie"):
            C.incoh_dedisperse(f32(12, 4), d, 8)
    with pytest.raises(RuntimeError, match="float32"):
        C.incoh_dedisperse(f32(12, 4).double(), i32(2, 4), 8)
    with pytest.raises(RuntimeError, match="int32"):
        C.incoh_dedisperse(f32(12, 4), i32(2, 4).long(), 8)
    with pytest.raises(RuntimeError, match="contiguous"):
        C.incoh_dedisperse(f32(12, 8)[:, ::2], i32(2, 4), 8)
    with pytest.raises(RuntimeError, match="contiguous"):
        C.incoh_dedisperse(f32(12, 4), i32(2, 8)[:, ::2], 8)
    with pytest.raises(RuntimeError, match="channels"):
        C.incoh_dedisperse(f32(12, 4), i32(2, 5), 8)
    with pytest.raises(RuntimeError, match="R must be"):
        C.incoh_detect(f32(3, 1), 6.0, 4)
    with pytest.raises(RuntimeError, match="R must be"):
        C.incoh_detect(f32(1, C.INCOH_MAX_ROWS + 1), 6.0, 4)
    with pytest.raises(RuntimeError, match="float32"):
        C.incoh_detect(f32(3, 8).double(), 6.0, 4)
    with pytest.raises(RuntimeError, match="contiguous"):
        C.incoh_detect(f32(3, 16)[:, ::2], 6.0, 4)
    with pytest.raises(RuntimeError, match="max_boxcar"):
        C.incoh_detect(f32(3, 8), 6.0, 0)


@pytest.mark.parametrize("kw,match", [
    (dict(offsets=[]), "offsets"),
    (dict(offsets=[0.0] * 1025), "offsets"),
    (dict(rows=1), "rows per block"),
    (dict(rows=16385), "rows per block"),
    (dict(offsets=[1e9]), "delay"),           # D_max > 2^20
    # D_max = 3.4e5 rows fits, its 2.8 GB of history do not
    (dict(offsets=[2e6], channels=2048, foff=-0.03), "cap"),
    (dict(foff=4.0, offsets=[100.0]), "delay"),  # ascending frequency
    (dict(max_boxcar=0), "max_boxcar"),
])
def test_search_constructor_rejections(C, kw, match):
    args = dict(rows=8, channels=16, fch1=1463.5, foff=-4.0, tsamp=1e-3,
                offsets=[1.0], snr_threshold=6.0, max_boxcar=4)
    args.update(kw)
    with pytest.raises(RuntimeError, match=match):
        C.IncoherentSearch(**args)
    with pytest.raises(ValueError):
        ref.CpuIncoherentSearch(
            args["rows"], args["channels"], args["fch1"], args["foff"],
            args["tsamp"], args["offsets"], args["snr_threshold"],
            args["max_boxcar"])


def test_submit_plane_rejects_wrong_planes(C):
    gpu = C.IncoherentSearch(rows=8, channels=16, fch1=1463.5, foff=-4.0,
                             tsamp=1e-3, offsets=[1.0], snr_threshold=6.0,
                             max_boxcar=4)
    with pytest.raises(RuntimeError, match="plane must be"):
        gpu.submit_plane(torch.zeros(8, 15).cuda())
    with pytest.raises(RuntimeError, match="plane must be"):
        gpu.submit_plane(torch.zeros(8, 16, dtype=torch.float64).cuda())
    with pytest.raises(RuntimeError, match="contiguous"):
        gpu.submit_plane(torch.zeros(8, 32).cuda()[:, ::2])
    with pytest.raises(RuntimeError, match="GPU"):
        gpu.submit_plane(torch.zeros(8, 16))


# ---- 6. applications ----

OFFSETS = "-2,-1,0,1,2,3,4"


def test_main_gpu_writes_the_injected_offset(tmp_path):
    from srtb_amd.main import main
    from tests.test_incoherent_cpu import (APP_ARGS, check_candidates,
                                           offset_pulse_recording)
    rec = tmp_path / "rec.bin"
    offset_pulse_recording(rec)
    out = tmp_path / "gpu.cand"
    rc = main(APP_ARGS + [
        "--device", "cuda", "--input_file_path", str(rec),
        "--incoherent_dm_offsets", OFFSETS,
        "--incoherent_output_path", str(out),
        "--baseband_output_file_prefix", f"{tmp_path}/g_"])
    assert rc == 0
    check_candidates(out)


def test_srtb_backend_writes_the_same_candidates_as_main(tmp_path):
    import os
    import subprocess
    from srtb_amd.main import main
    from tests.test_incoherent_cpu import (APP_ARGS, check_candidates,
                                           offset_pulse_recording)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    binary = os.path.join(root, "bin", "srtb-backend")
    assert os.path.exists(binary), "native binaries not built"
    rec = tmp_path / "rec.bin"
    offset_pulse_recording(rec)
    fil = tmp_path / "both.fil"  # the file and the search share the plane
    args = APP_ARGS + ["--input_file_path", str(rec),
                       "--incoherent_dm_offsets", OFFSETS,
                       "--filterbank_output_path", str(fil),
                       "--filterbank_nbits", "32"]
    py_out, cc_out = tmp_path / "py.cand", tmp_path / "cc.cand"
    assert main(args + ["--device", "cuda",
                        "--incoherent_output_path", str(py_out),
                        "--baseband_output_file_prefix",
                        f"{tmp_path}/p_"]) == 0
    py_fil = len(fil.read_bytes())
    run = subprocess.run(
        ["timeout", "-k", "10", "120", binary] + args +
        ["--incoherent_output_path", str(cc_out),
         "--baseband_output_file_prefix", f"{tmp_path}/c_"],
        capture_output=True, text=True, timeout=150)
    assert run.returncode == 0, run.stderr
    check_candidates(py_out)
    assert cc_out.read_bytes() == py_out.read_bytes()
    # the two apps' planes agree to the last bits, not in them (their engines
    # are configured alike but not identically): same size here, no more
    assert len(fil.read_bytes()) == py_fil > 0


def test_srtb_backend_rejects_the_exclusions(tmp_path):
    import os
    import subprocess
    from tests.test_incoherent_cpu import APP_ARGS
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    binary = os.path.join(root, "bin", "srtb-backend")
    base = [binary] + APP_ARGS + ["--input_file_path", "none.bin",
                                  "--incoherent_dm_offsets", "0,1"]
    for extra, word in [
            ([], "need each other"),
            (["--incoherent_output_path", "c.cand",
              "--dm_trial_list", "59,60"], "dm_trial_list"),
            (["--incoherent_output_path", "c.cand",
              "--filterbank_polarization", "I"], "filterbank_polarization")]:
        run = subprocess.run(base + extra, capture_output=True, text=True,
                             timeout=60, cwd=tmp_path)
        assert run.returncode == 2, (extra, run.stdout, run.stderr)
        assert word in run.stdout + run.stderr
