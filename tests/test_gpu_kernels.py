"""GPU numerics tests: every HIP kernel vs the NumPy/torch fp32 oracle."""

import numpy as np
import pytest
import torch

from srtb_amd import ref

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def C():
    from srtb_amd.ops import native
    torch.cuda.set_device(0)
    return native()


def to_gpu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


# ---------------- unpack ----------------

@pytest.mark.parametrize("nbits", [1, 2, 4, 8, -8])
def test_unpack_matches_oracle(C, nbits):
    rng = np.random.default_rng(1)
    raw = rng.integers(0, 256, 1 << 12, dtype=np.uint8)
    expect = ref.unpack(raw, nbits)
    out = C.unpack(to_gpu(raw), nbits, expect.size).cpu().numpy()
    np.testing.assert_array_equal(out, expect)


@pytest.mark.parametrize("nbits", [1, 2, 4])
@pytest.mark.parametrize("n_bytes", [300, 255, 256 + 17])
def test_unpack_subbyte_tail(C, nbits, n_bytes):
    """Non-multiple-of-256-byte inputs take the wave-block main kernel PLUS
    the byte-per-lane tail kernel; pow2-sized tests never exercise the
    seam."""
    rng = np.random.default_rng(10 * nbits + n_bytes)
    raw = rng.integers(0, 256, n_bytes, dtype=np.uint8)
    expect = ref.unpack(raw, nbits)
    out = C.unpack(to_gpu(raw), nbits, expect.size).cpu().numpy()
    np.testing.assert_array_equal(out, expect)
    # and with a window, which the tail kernel must index absolutely
    w = ref.window_coefficients("hann", expect.size)
    expect_w = ref.unpack(raw, nbits, window=w)
    out_w = C.unpack(to_gpu(raw), nbits, expect.size, to_gpu(w)).cpu().numpy()
    np.testing.assert_allclose(out_w, expect_w, rtol=1e-6)


def test_unpack_16bit(C):
    rng = np.random.default_rng(2)
    raw = rng.integers(0, 256, 1 << 12, dtype=np.uint8)
    for b in (16, -16):
        expect = ref.unpack(raw, b)
        out = C.unpack(to_gpu(raw), b, expect.size).cpu().numpy()
        np.testing.assert_array_equal(out, expect)


@pytest.mark.parametrize("nbits", [2, 8, -16, 32])
def test_unpack_with_window(C, nbits):
    """Window fusion must apply to EVERY sample format (the 16/32-bit cast
    cases once hardcoded it off)."""
    rng = np.random.default_rng(3)
    raw = rng.integers(0, 256, 4096, dtype=np.uint8)
    expect_plain = ref.unpack(raw, nbits)
    w = ref.window_coefficients("hamming", expect_plain.size)
    expect = ref.unpack(raw, nbits, window=w)
    out = C.unpack(to_gpu(raw), nbits, expect.size, to_gpu(w)).cpu().numpy()
    np.testing.assert_allclose(out, expect, rtol=1e-5, atol=1e-3)


def test_unpack_2pol_kinds(C):
    rng = np.random.default_rng(4)
    raw = rng.integers(0, 256, 1 << 12, dtype=np.uint8)
    p0, p1 = ref.unpack_interleaved_2pol(raw)
    g0, g1 = C.unpack_2pol(to_gpu(raw), "interleave")
    np.testing.assert_array_equal(g0.cpu().numpy(), p0)
    np.testing.assert_array_equal(g1.cpu().numpy(), p1)
    p0, p1 = ref.unpack_naocpsr_snap1(raw)
    g0, g1 = C.unpack_2pol(to_gpu(raw), "naocpsr_snap1")
    np.testing.assert_array_equal(g0.cpu().numpy(), p0)
    np.testing.assert_array_equal(g1.cpu().numpy(), p1)


@pytest.mark.parametrize("ns", [2, 4])
def test_unpack_gznupsr(C, ns):
    rng = np.random.default_rng(5)
    raw = rng.integers(0, 256, 1 << 12, dtype=np.uint8)
    expect = ref.unpack_gznupsr_a1(raw, n_streams=ns)
    outs = C.unpack_gznupsr_a1(to_gpu(raw), ns)
    for e, o in zip(expect, outs):
        np.testing.assert_array_equal(o.cpu().numpy(), e)


# ---------------- reductions ----------------

def test_mean_power(C):
    rng = np.random.default_rng(6)
    x = (rng.normal(size=1 << 16) + 1j * rng.normal(size=1 << 16)
         ).astype(np.complex64)
    m = C.mean_power(to_gpu(x)).cpu().item()
    expect = np.mean(np.abs(x.astype(np.complex128)) ** 2)
    assert abs(m - expect) < 1e-6 * expect


def test_sum_sumsq(C):
    rng = np.random.default_rng(7)
    x = rng.normal(size=12345).astype(np.float32)
    s = C.sum_sumsq(to_gpu(x)).cpu().numpy()
    np.testing.assert_allclose(s[0], x.astype(np.float64).sum(), rtol=1e-10)
    np.testing.assert_allclose(s[1], (x.astype(np.float64) ** 2).sum(),
                               rtol=1e-10)


# ---------------- RFI s1 / dedispersion ----------------

def test_rfi_s1(C):
    rng = np.random.default_rng(8)
    n, s = 1 << 14, 1 << 8
    spec = (rng.normal(size=n) + 1j * rng.normal(size=n)).astype(np.complex64)
    spec[1000] = 500.0
    expect = ref.rfi_mitigate_s1(spec, 10.0, s)
    g = to_gpu(spec)
    C.rfi_s1(g, 10.0, s)
    np.testing.assert_allclose(g.cpu().numpy(), expect, rtol=2e-5, atol=1e-6)


def test_zap_bins(C):
    spec = np.ones(256, dtype=np.complex64)
    g = to_gpu(spec)
    C.zap_bins(g, 10, 20)
    out = g.cpu().numpy()
    assert (out[10:21] == 0).all()
    assert out[9] == 1 and out[21] == 1


def test_dedisperse_vs_oracle(C):
    rng = np.random.default_rng(9)
    n = 1 << 14
    spec = (rng.normal(size=n) + 1j * rng.normal(size=n)).astype(np.complex64)
    f_min, bw, dm = 1437.0, -64.0, -478.8
    f_c, df = f_min + bw, bw / n
    expect = ref.coherent_dedisperse(spec, f_min, f_c, df, dm)
    g = to_gpu(spec)
    C.dedisperse(g, f_min, f_c, df, dm)
    np.testing.assert_allclose(g.cpu().numpy(), expect, rtol=1e-4, atol=1e-4)


def test_phase_table(C):
    n = 1 << 12
    f_min, bw, dm = 1000.0, 500.0, 478.8
    f_c, df = f_min + bw, bw / n
    expect = ref.dedisp_phase_factors(n, f_min, f_c, df, dm)
    t = C.dedisp_phase_table(n, f_min, f_c, df, dm,
                             torch.device("cuda")).cpu().numpy()
    np.testing.assert_allclose(t, expect, atol=2e-6)


def test_fused_equals_sequential(C):
    rng = np.random.default_rng(10)
    n, s = 1 << 14, 1 << 8
    spec = (rng.normal(size=n) + 1j * rng.normal(size=n)).astype(np.complex64)
    spec[77] = 300.0
    f_min, bw, dm = 1437.0, -64.0, -478.8
    f_c, df = f_min + bw, bw / n
    # sequential oracle
    e = ref.rfi_mitigate_s1(spec, 1.5, s)
    e[100:121] = 0
    e = ref.coherent_dedisperse(e, f_min, f_c, df, dm)
    g = to_gpu(spec)
    C.rfi_dedisperse_fused(g, True, 1.5, s, [[100, 120]], f_min, f_c, df, dm)
    np.testing.assert_allclose(g.cpu().numpy(), e, rtol=1e-4, atol=1e-5)


def test_fused_with_table_matches_fly(C):
    rng = np.random.default_rng(11)
    n, s = 1 << 13, 1 << 7
    spec = (rng.normal(size=n) + 1j * rng.normal(size=n)).astype(np.complex64)
    f_min, bw, dm = 1400.0, 64.0, 100.0
    f_c, df = f_min + bw, bw / n
    g1 = to_gpu(spec)
    g2 = to_gpu(spec)
    tab = C.dedisp_phase_table(n, f_min, f_c, df, dm, torch.device("cuda"))
    C.rfi_dedisperse_fused(g1, True, 5.0, s, [], f_min, f_c, df, dm)
    C.rfi_dedisperse_fused(g2, True, 5.0, s, [], f_min, f_c, df, dm, tab)
    np.testing.assert_allclose(g1.cpu().numpy(), g2.cpu().numpy(), atol=1e-6)


# ---------------- SK ----------------

def test_sk_row_stats(C):
    rng = np.random.default_rng(12)
    wf = (rng.normal(size=(32, 512)) + 1j * rng.normal(size=(32, 512))
          ).astype(np.complex64)
    out = C.sk_row_stats(to_gpu(wf)).cpu().numpy()
    p = np.abs(wf.astype(np.complex128)) ** 2
    np.testing.assert_allclose(out[:, 0], p.sum(axis=1), rtol=1e-4)
    np.testing.assert_allclose(out[:, 1], (p * p).sum(axis=1), rtol=1e-4)


def test_sk_mitigate(C):
    rng = np.random.default_rng(13)
    wf = (rng.normal(size=(32, 2048)) + 1j * rng.normal(size=(32, 2048))
          ).astype(np.complex64)
    wf[7, :] = 0
    wf[7, ::100] = 50.0
    expect = ref.rfi_mitigate_sk(wf, 1.05)
    g = to_gpu(wf)
    flags, zero_count = C.sk_mitigate(g, 1.05)
    out = g.cpu().numpy()
    fl = flags.cpu().numpy()
    assert fl[7] == 1
    assert (out[7] == 0).all()
    ez = (np.abs(expect).sum(axis=1) == 0)
    np.testing.assert_array_equal(fl.astype(bool), ez)
    np.testing.assert_allclose(out, expect, rtol=1e-5)
    assert zero_count.cpu().item() == int(ez.sum())


# ---------------- detection ----------------

def test_time_series(C):
    rng = np.random.default_rng(14)
    wf = (rng.normal(size=(16, 256)) + 1j * rng.normal(size=(16, 256))
          ).astype(np.complex64)
    expect = ref.time_series_sum(wf, 200)
    out = C.time_series(to_gpu(wf), None, 200).cpu().numpy()
    np.testing.assert_allclose(out, expect, rtol=1e-4)


def test_subtract_mean_and_count(C):
    rng = np.random.default_rng(15)
    ts = rng.normal(size=1 << 14).astype(np.float32)
    ts[100] = 50.0
    g = to_gpu(ts)
    C.subtract_mean(g)
    e = ts - ts.mean(dtype=np.float64)
    np.testing.assert_allclose(g.cpu().numpy(), e, atol=1e-4)
    cnt, thr = C.count_signal(g, 6.0)
    ecnt, ethr = ref.count_signal(e.astype(np.float32), 6.0)
    assert cnt.cpu().item() == ecnt
    np.testing.assert_allclose(thr.cpu().item(), ethr, rtol=1e-5)


def test_inclusive_scan(C):
    rng = np.random.default_rng(16)
    for n in (1, 63, 2048, 2049, 1 << 16, (1 << 18) - 7):
        x = rng.normal(size=n).astype(np.float32)
        out = C.inclusive_scan(to_gpu(x)).cpu().numpy()
        expect = np.cumsum(x, dtype=np.float64)
        np.testing.assert_allclose(out, expect, rtol=1e-3, atol=2e-2)


def test_boxcar(C):
    rng = np.random.default_rng(17)
    ts = rng.normal(size=4096).astype(np.float32)
    cum = C.inclusive_scan(to_gpu(ts))
    box = C.boxcar(cum, 8).cpu().numpy()
    expect = ref.boxcar_series(ts, 8)
    np.testing.assert_allclose(box, expect, rtol=1e-3, atol=2e-2)


# ---------------- detection and SK, exact ----------------
#
# Inputs are small integers, so every float32 partial sum is an integer
# below 2^24 and exact in any order: the kernels must reproduce the float64
# sums bit for bit.

U = 2.0 ** -24


def int_waterfall(rows, length, amp, seed):
    rng = np.random.default_rng(seed)
    re = rng.integers(-amp, amp + 1, size=(rows, length))
    im = rng.integers(-amp, amp + 1, size=(rows, length))
    return (re + 1j * im).astype(np.complex64)


def ts_flag_pattern(kind, rows):
    """none; one whole chunk of the two-stage kernel (its second: rows
    [per, 2 per) with per = ceil(rows / min(64, rows))) plus the last row;
    every third row; all rows."""
    f = np.zeros(rows, dtype=np.uint8)
    if kind == "chunk":
        per = -(-rows // min(64, rows))
        f[per:2 * per] = 1
        f[-1] = 1
    elif kind == "third":
        f[::3] = 1
    elif kind == "all":
        f[:] = 1
    return None if kind == "none" else f


@pytest.mark.parametrize("flags", ["none", "chunk", "third", "all"])
@pytest.mark.parametrize("rows,length,ts_count", [
    (16, 256, 200),
    (70, 514, 511),      # odd ts_count: the last column has no pair;
                         # 70 rows over 64 chunks: the last chunks are empty
    (3, 8, 7),           # fewer rows than chunks
    (130, 4098, 4097),   # 9 column blocks, 3 rows per chunk, 130 = 43 * 3 + 1
    (5, 255, 255),       # odd row length: the single-pass fallback
])
def test_time_series_exact(C, rows, length, ts_count, flags):
    wf = int_waterfall(rows, length, 15, seed=rows + length)
    f = ts_flag_pattern(flags, rows)
    p = wf.real.astype(np.float64) ** 2 + wf.imag.astype(np.float64) ** 2
    if f is not None:
        p[f != 0] = 0
    want = p[:, :ts_count].sum(axis=0)
    assert want.max() < 2 ** 24
    got = C.time_series(to_gpu(wf), None if f is None else to_gpu(f),
                        ts_count).cpu().numpy()
    assert got.dtype == np.float32 and got.shape == (ts_count,)
    np.testing.assert_array_equal(got, want.astype(np.float32))
    assert (want > 0).any() or flags == "all"


@pytest.mark.parametrize("n", [1, 2047, 2048, 2049, 2048 * 256,
                               2048 * 256 + 1, 2048 * 300 + 5])
def test_inclusive_scan_exact(C, n):
    """More than 256 blocks of 2048 take the serial-chunk branch of the
    block-sums kernel.  Every partial sum of the scan is the sum of a
    contiguous range, a difference of two cumulative sums."""
    rng = np.random.default_rng(n)
    x = rng.integers(-3, 4, size=n).astype(np.float32)
    want = np.cumsum(x.astype(np.float64))
    assert np.abs(want).max() < 2 ** 23
    got = C.inclusive_scan(to_gpu(x)).cpu().numpy()
    np.testing.assert_array_equal(got, want.astype(np.float32))


LADDER_LENGTHS = [2 << k for k in range(12)]  # 2 .. 4096, the kernel's 12


@pytest.mark.parametrize("ts_count", [5, 64, 2049, 300001])
def test_boxcar_ladder(C, ts_count):
    """Integer series with planted spikes: every box value is an exact
    integer.  Lengths >= ts_count (and == ts_count at 64) have no window."""
    snr = 6.0
    rng = np.random.default_rng(ts_count)
    ts = rng.integers(-3, 4, size=ts_count).astype(np.float64)
    for pos, amp in [(3, 60), (ts_count // 2, 100), (ts_count - 2, 250)]:
        ts[pos] += amp
        ts[(pos * 7 + 1) % ts_count:][:9] += amp // 10  # a wide, low one
    cum = np.cumsum(ts)
    assert np.abs(cum).max() < 2 ** 23
    thr, counts = C.boxcar_ladder(to_gpu(cum.astype(np.float32)),
                                  LADDER_LENGTHS, snr)
    thr, counts = thr.cpu().numpy(), counts.cpu().numpy()
    assert thr.dtype == np.float32 and counts.dtype == np.int32
    assert thr.shape == counts.shape == (12,)
    seen = 0
    for k, b in enumerate(LADDER_LENGTHS):
        if b >= ts_count:
            assert counts[k] == 0, (b, counts[k])
            continue
        box = cum[b:] - cum[:-b]
        want = np.float32(snr) * np.float32(np.sqrt((box * box).sum()
                                                    / box.size))
        assert abs(float(thr[k]) - float(want)) <= 2 * U * float(want), \
            (b, thr[k], want)
        n = int((box.astype(np.float32) > thr[k]).sum())
        assert counts[k] == n, (b, counts[k], n)
        seen += n
    # (a series of a few dozen samples cannot hold a 6-sigma window)
    assert seen > 0 or ts_count < 2049


@pytest.mark.parametrize("rows,length", [(5, 513), (3, 2), (4, 1)])
def test_sk_row_stats_exact(C, rows, length):
    """An odd length takes the scalar kernel (rows are not 16-byte aligned);
    length 2 is one float4 per row."""
    wf = int_waterfall(rows, length, 3, seed=length)
    p = wf.real.astype(np.float64) ** 2 + wf.imag.astype(np.float64) ** 2
    s2, s4 = p.sum(axis=1), (p * p).sum(axis=1)
    assert s4.max() < 2 ** 24
    got = C.sk_row_stats(to_gpu(wf)).cpu().numpy()
    np.testing.assert_array_equal(got[:, 0], s2.astype(np.float32))
    np.testing.assert_array_equal(got[:, 1], s4.astype(np.float32))


# The final DIF pass of a length-L plan runs n-point transforms, F to a
# workgroup; workgroup w of a row stores the columns J + k L/n with
# J in [w F, (w + 1) F) and k in [0, n): the first is w F, the last
# L - L/n + w F + F - 1.
#   L = 8192:  n = 256, F = 16, 2 workgroups per row:
#              first 0, 16; last 8175, 8191
#   L = 16384: n = 64, F = 32, 8 workgroups per row:
#              first 0, 32, ..., 224; last 16159, 16191, ..., 16383
#   L = 4096:  the single-pass DIF, one workgroup per row (not an engine
#              shape: the waterfall FFT takes the wave kernel below 4096 and
#              column passes above)
DIF_SHAPE = {8192: (256, 16), 16384: (64, 32), 4096: (4096, 1)}


@pytest.mark.parametrize("rows,L", [(64, 8192), (64, 16384), (8, 4096)])
def test_native_fft_sk_owns_every_element_once(C, rows, L):
    """Row r is a tone whose backward transform is one spike of size L at
    column j_r: a workgroup of the DIF epilogue that drops or doubles the
    column, or a partial that lands in another row, changes that row's sums
    by a factor of order 1."""
    n, F = DIF_SHAPE[L]
    wgs = L // n // F
    cols = [0, 1, 255, 256, L // 2 - 1, L // 2, L - 1]
    for w in range(wgs):
        cols += [w * F, L - L // n + w * F + F - 1]
    cols = list(dict.fromkeys(cols))[:rows]
    rng = np.random.default_rng(L)
    j = np.array(cols + list(rng.integers(0, L, size=rows - len(cols))))
    k = np.arange(L)
    x = np.exp(-2j * np.pi * ((j[:, None] * k[None, :]) % L) / L)
    x += 1e-3 * (rng.normal(size=(rows, L)) + 1j * rng.normal(size=(rows, L)))
    xt = to_gpu(x.astype(np.complex64))
    out, stats = C.native_fft_sk(xt)
    out, stats = out.cpu().numpy(), stats.cpu().numpy().astype(np.float64)
    plain = C.native_fft(xt, 1).cpu().numpy()
    assert np.array_equal(out.view(np.uint32), plain.view(np.uint32))
    assert np.array_equal(np.abs(out).argmax(axis=1), j)
    p = out.real.astype(np.float64) ** 2 + out.imag.astype(np.float64) ** 2
    s2, s4 = p.sum(axis=1), (p * p).sum(axis=1)
    assert (s2 > 0.9 * L * L).all()
    r2 = np.abs(stats[:, 0] - s2) / s2 / ((L + 4) * U)
    r4 = np.abs(stats[:, 1] - s4) / s4 / ((L + 8) * U)
    print(f"L {L}: max |err| / bound: s2 {r2.max():.4f} s4 {r4.max():.4f}")
    assert r2.max() <= 1.0 and r4.max() <= 1.0, (r2, r4)


def test_native_fft_sk_rejects_a_plan_without_epilogue(C):
    x = torch.zeros(4, 1024, dtype=torch.complex64).cuda()
    with pytest.raises(RuntimeError):  # the wave kernel has no SK epilogue
        C.native_fft_sk(x)


# ---------------- display ----------------

def test_resample_power(C):
    rng = np.random.default_rng(18)
    wf = (rng.normal(size=(64, 256)) + 1j * rng.normal(size=(64, 256))
          ).astype(np.complex64)
    out = C.resample_power(to_gpu(wf), 16, 32).cpu().numpy()
    expect = ref.resample_power_2d(np.abs(wf.astype(np.complex128)) ** 2, 16, 32)
    np.testing.assert_allclose(out, expect, rtol=1e-4)


def test_normalize_and_pixmap(C):
    rng = np.random.default_rng(19)
    img = rng.random(1000).astype(np.float32)
    g = to_gpu(img)
    C.normalize_by_mean(g)
    expect = ref.normalize_by_mean(img)
    np.testing.assert_allclose(g.cpu().numpy(), expect, rtol=1e-5)
    pix = C.generate_pixmap(g, ref.COLOR_0, ref.COLOR_1,
                            ref.COLOR_OVERFLOW).cpu().numpy().view(np.uint32)
    epix = ref.generate_pixmap(g.cpu().numpy())
    np.testing.assert_array_equal(pix, epix)


def test_running_mean(C):
    rng = np.random.default_rng(20)
    data = rng.random((64, 8)).astype(np.float32)
    out, ave = C.running_mean(to_gpu(data), 16)
    a0 = ref.running_mean_init_average(data, 16)
    eout, eave = ref.running_mean(data, 16, a0)
    np.testing.assert_array_equal(out.cpu().numpy(), eout)
    np.testing.assert_allclose(ave.cpu().numpy(), eave, rtol=1e-4)


def test_correlate(C):
    rng = np.random.default_rng(21)
    f1 = (rng.normal(size=512) + 1j * rng.normal(size=512)).astype(np.complex64)
    f2 = (rng.normal(size=512) + 1j * rng.normal(size=512)).astype(np.complex64)
    corr, mag = C.correlate(to_gpu(f1), to_gpu(f2), 0.25)
    expect = ref.correlate_spectra(f1, f2, 0.25)
    np.testing.assert_allclose(corr.cpu().numpy(), expect, rtol=1e-4, atol=1e-5)
    np.testing.assert_allclose(mag.cpu().numpy(), np.abs(expect), rtol=1e-4,
                               atol=1e-5)


@pytest.mark.parametrize("normalize", [False, True])
def test_sk_v1_mitigate(C, normalize):
    rng = np.random.default_rng(30)
    M, bins = 256, 96  # bins deliberately non-pow2
    wf = (rng.normal(size=(M, bins)) + 1j * rng.normal(size=(M, bins))
          ).astype(np.complex64)
    wf[:, 5] = 0
    wf[::40, 5] = 25.0
    expect = ref.rfi_mitigate_sk_v1(wf, 1.05, normalize=normalize)
    g = to_gpu(wf)
    C.sk_v1_mitigate(g, 1.05, normalize)
    np.testing.assert_allclose(g.cpu().numpy(), expect, rtol=1e-4, atol=1e-4)
