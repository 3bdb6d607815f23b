"""The engine's back half, stage by stage, on a block that makes every stage
decide something (backhalf_block.py): spectral-kurtosis sums (fused into the
backward FFT's DIF store at L >= 8192) -> flags -> zero_count -> lazy zap ->
time series -> raw threshold and count -> cumulative sum -> boxcar ladder.

Every expected value is computed in float64 from the engine's OWN previous
stage, so no tolerance has to absorb the FFT: the bounds are the worst case
of the float32 arithmetic of that one stage, u = 2^-24.

Shapes: N = 2^18 with S = 16 (L = 8192, backward plan [32] + 256, 2 DIF
workgroups per row) and S = 8 (L = 16384, [16, 16] + 64, 8 per row): the
smallest with a fused first pass and a fused DIF epilogue of each final
length.  S = 16 also runs on the rocFFT waterfall (fft_backend 1 and 2),
where the unfused kernels must satisfy the same assertions.
"""

import numpy as np
import pytest
import torch

import backhalf_block as bb

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
N = bb.N

# id: (S, fft_backend, windowed)
CASES = {
    "S16-native": (16, 0, False),
    "S8-native": (8, 0, False),
    "S16-hipfft": (16, 1, False),
    "S16-auto": (16, 2, False),
    "S16-native-hamming": (16, 0, True),
}
PLAIN = [k for k, v in CASES.items() if not v[2]]


@pytest.fixture(scope="module")
def C():
    from srtb_amd.ops import native
    torch.cuda.set_device(0)
    return native()


def make_engine(C, S, fft, windowed, **kw):
    args = dict(
        n=N, nbits=-8, channels=S, freq_low=bb.FREQ_LOW,
        bandwidth=bb.BANDWIDTH, sample_rate=bb.SAMPLE_RATE, dm=bb.DM,
        rfi_threshold=bb.RFI_THRESHOLD,
        sk_threshold=bb.WINDOWED_SK_THRESHOLD if windowed else bb.SK_THRESHOLD,
        snr_threshold=bb.SNR_THRESHOLD, max_boxcar=bb.MAX_BOXCAR,
        nsamps_reserved=bb.reserved(S), zap_ranges=bb.ZAP,
        use_phase_table=False, enable_rfi_s1=True, enable_sk=True, n_slots=2,
        fft_backend=fft, window_kind=2 if windowed else 0)
    args.update(kw)
    return C.PipelineEngine(**args)


def products(eng, slot, res):
    """Everything the assertions read, copied to the host.  The un-zapped
    waterfall first: the default waterfall() read applies the lazy zap."""
    p = {
        "res": res,
        "wf": eng.waterfall(slot, zap=False).cpu().numpy(),
        "stats": eng.sk_stats(slot).cpu().numpy(),
        "flags": eng.sk_flags(slot).cpu().numpy(),
        "ts": eng.time_series(slot).cpu().numpy(),
        "cum": eng.cumsum(slot).cpu().numpy(),
    }
    p["wf_zapped"] = eng.waterfall(slot).cpu().numpy()
    return p


_cache = {}


@pytest.fixture(scope="module", autouse=True)
def _drop_engines():
    yield
    _cache.clear()


def get_case(C, key):
    """One engine per case and one block through its first slot, shared by
    the tests."""
    if key not in _cache:
        S, fft, windowed = CASES[key]
        raw_np = bb.make_noise_block() if windowed else bb.make_block(S)
        raw = torch.from_numpy(raw_np).pin_memory()
        eng = make_engine(C, S, fft, windowed)
        slot = eng.submit(raw)
        res = eng.wait(slot)
        c = products(eng, slot, res)
        c.update(key=key, S=S, L=N // 2 // S, fft=fft, windowed=windowed,
                 raw=raw, eng=eng, slot=slot, ts_count=eng.ts_count,
                 thr=bb.sk_thresholds(
                     N // 2 // S, bb.WINDOWED_SK_THRESHOLD if windowed
                     else bb.SK_THRESHOLD))
        assert c["wf"].shape == (S, c["L"])
        assert c["ts_count"] == c["L"] - 3 and c["ts_count"] % 2 == 1
        _cache[key] = c
    return _cache[key]


@pytest.fixture(params=list(CASES))
def case(C, request):
    return get_case(C, request.param)


@pytest.fixture(params=PLAIN)
def plain(C, request):
    """The crafted block only: the windowed engine's input is noise."""
    return get_case(C, request.param)


def power64(wf):
    return wf.real.astype(np.float64) ** 2 + wf.imag.astype(np.float64) ** 2


# ---- 1. SK sums ----

def test_sk_sums(case):
    """Any summation order over L non-negative terms, each |x|^2 (|x|^4)
    carrying 2 (5) roundings of its own, stays within (L + 4) u of the exact
    s2 and (L + 8) u of the exact s4."""
    L = case["L"]
    p = power64(case["wf"])
    s2, s4 = p.sum(axis=1), (p * p).sum(axis=1)
    got = case["stats"].astype(np.float64)
    r2 = np.abs(got[:, 0] - s2) / s2 / ((L + 4) * U)
    r4 = np.abs(got[:, 1] - s4) / s4 / ((L + 8) * U)
    print(f"{case['key']}: B.1 max |err| / bound: s2 {r2.max():.4f} "
          f"s4 {r4.max():.4f} (bounds {(L + 4) * U:.3e}, {(L + 8) * U:.3e})")
    assert (s2 > 0).all()
    assert r2.max() <= 1.0, (r2, got[:, 0], s2)
    assert r4.max() <= 1.0, (r4, got[:, 1], s4)


# ---- 2. flags ----

def test_sk_flags(case):
    L, (lo, hi) = case["L"], case["thr"]
    p = power64(case["wf"])
    s2, s4 = p.sum(axis=1), (p * p).sum(axis=1)
    sk = L * s4 / (s2 * s2)
    want = (sk > hi) | (sk < lo) | (s2 == 0)
    # a row whose SK the float32 sums could carry across a threshold
    unsure = np.minimum(np.abs(sk - lo), np.abs(sk - hi)) <= 3 * (L + 8) * U * sk
    print(f"{case['key']}: SK {np.round(sk, 3)} lo' {lo} hi' {hi}")
    assert not unsure.any()
    np.testing.assert_array_equal(case["flags"], want.astype(np.uint8))
    assert 0 < want.sum() < case["S"]
    if not case["windowed"]:
        assert set(np.nonzero(want)[0]) == {bb.CHIRP_ROW,
                                            bb.tone_row(case["S"])}


# ---- 3. zero_count ----

def test_zero_count(case):
    flags = case["flags"].astype(bool)
    first_zero = power64(case["wf"][:, 0]) == 0
    assert case["res"]["zero_count"] == int((flags | first_zero).sum())


# ---- 4. lazy zap ----

def test_lazy_zap(case):
    flags = case["flags"].astype(bool)
    wf, z = case["wf"], case["wf_zapped"]
    assert (z[flags].view(np.uint32) == 0).all()  # +0.0, bit for bit
    assert np.array_equal(z[~flags].view(np.uint32), wf[~flags].view(np.uint32))
    assert (wf[flags] != 0).any()  # the chain itself left the rows alone
    # and the default read keeps returning the zapped waterfall
    again = case["eng"].waterfall(case["slot"]).cpu().numpy()
    assert np.array_equal(again.view(np.uint32), z.view(np.uint32))


# ---- 5. time series ----

def test_time_series(case):
    """S float32 additions of non-negative terms (two-stage or not), 2
    roundings per |x|^2, then the float32 mean and its subtraction."""
    S, n = case["S"], case["ts_count"]
    flags = case["flags"].astype(bool)
    raw = power64(case["wf"])[~flags, :n].sum(axis=0)
    want = raw - raw.mean()
    atol = (S + 6) * U * raw.max()
    err = np.abs(case["ts"].astype(np.float64) - want).max()
    print(f"{case['key']}: B.5 max |err| {err:.4e} bound {atol:.4e} "
          f"ratio {err / atol:.4f}")
    assert case["ts"].shape == (n,)
    assert err <= atol


# ---- 6. raw threshold and count ----

def counts_of(res):
    return dict(res["counts"])


def test_raw_threshold_and_count(plain):
    ts = plain["ts"]
    thr = plain["res"]["thresholds"][0]
    want = bb.SNR_THRESHOLD * np.sqrt((ts.astype(np.float64) ** 2).mean())
    assert abs(thr - want) <= 4 * U * want, (thr, want)
    n = int((ts > np.float32(thr)).sum())
    assert counts_of(plain["res"])[1] == n
    assert n > 0


# ---- 7. cumulative sum ----

def test_cumsum(plain):
    """Every element passes through at most 32 float32 additions in the
    two-level scan (8 serial, 8 Hillis-Steele steps, 1 exclusive, the block
    offsets' 8 + 1, and the final add), each bounded by sum |ts|."""
    ts = plain["ts"].astype(np.float64)
    want = np.cumsum(ts)
    atol = 32 * U * np.abs(ts).sum()
    err = np.abs(plain["cum"].astype(np.float64) - want).max()
    print(f"{plain['key']}: B.7 max |err| {err:.4e} bound {atol:.4e} "
          f"ratio {err / atol:.4f}")
    assert err <= atol


# ---- 8. ladder ----

def test_ladder(plain):
    cum = plain["cum"]
    assert cum.dtype == np.float32
    lengths = bb.boxcar_lengths(plain["ts_count"])
    counts = counts_of(plain["res"])
    assert sorted(counts) == [1] + lengths
    for k, b in enumerate(lengths):
        box = cum[b:] - cum[:-b]  # float32, as the kernel forms it
        assert box.dtype == np.float32
        thr = plain["res"]["thresholds"][1 + k]
        want = bb.SNR_THRESHOLD * np.sqrt((box.astype(np.float64) ** 2).mean())
        assert abs(thr - want) <= 4 * U * want, (b, thr, want)
        n = int((box > np.float32(thr)).sum())
        assert counts[b] == n, (b, counts[b], n)
        assert n > 0, b


# ---- 9. slots and graphs ----

def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.uint32),
                                                 b.view(np.uint32))


def assert_same_products(a, b):
    assert same_bits(a["stats"], b["stats"])
    assert np.array_equal(a["flags"], b["flags"])
    assert same_bits(a["ts"], b["ts"])
    assert same_bits(a["cum"], b["cum"])
    assert a["res"]["zero_count"] == b["res"]["zero_count"]
    assert a["res"]["counts"] == b["res"]["counts"]
    assert a["res"]["thresholds"] == b["res"]["thresholds"]


def test_second_slot_is_bit_identical(plain):
    eng = plain["eng"]
    slot = eng.submit(plain["raw"])
    assert slot != plain["slot"]
    res = eng.wait(slot)
    assert_same_products(plain, products(eng, slot, res))
    # bring the engine back to where the other tests expect it
    assert eng.submit(plain["raw"]) == plain["slot"]
    eng.wait(plain["slot"])
    eng.waterfall(plain["slot"])


def test_hip_graph_is_bit_identical(C, plain):
    """Per slot: a direct submission, then the captured one; the third
    submission of the engine is slot 0's captured chain, the fifth replays
    it."""
    eng = make_engine(C, plain["S"], plain["fft"], False, use_hip_graph=True)
    for i in range(5):
        slot = eng.submit(plain["raw"])
        res = eng.wait(slot)
        if i in (2, 4):
            assert slot == 0
            assert_same_products(plain, products(eng, slot, res))
