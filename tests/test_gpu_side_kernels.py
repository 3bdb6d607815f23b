"""GPU tests, per element: the kernels outside the block chain.

Display path (resample_power_2d, normalize_by_mean, generate_pixmap), the
correlator's kernels (correlate_pointwise, complex_abs), running_mean, SK
method 1, the standalone spectrum stage (rfi_s1, zap_bins, dedisperse,
dedisp_phase_table, rfi_dedisperse_fused in place) and the two reductions
(mean_power, sum_sumsq).

Oracles are float64 NumPy on the same float32 input.  Wherever small
integers, dyadic scales and power-of-two counts make the kernel's float32
arithmetic exact, the test asserts bit equality; every other limit is derived
in the test's docstring from the kernel's operation count, in units of
u = 2^-24, the largest relative error of one float32 rounding.

grid_for() caps an elementwise launch at 4096 x 256 = 2^20 threads: "past
the cap" is PAST = 2^20 + 2^12 + 3 elements (or the next size a kernel can
take), where the grid-stride loops make a second, ragged trip.
"""

import numpy as np
import pytest
import torch

import test_gpu_dedisp_poly as dp
from srtb_amd import ref

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
CAP = 1 << 20
PAST = CAP + (1 << 12) + 3


@pytest.fixture(scope="module")
def C():
    from srtb_amd.ops import native
    torch.cuda.set_device(0)
    return native()


def to_gpu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def bits(a):
    """The array's bit patterns, so that -0.0 != 0.0 and NaN == NaN."""
    a = np.ascontiguousarray(a)
    if a.dtype == np.complex64:
        a = a.view(np.float32)
    return a.view(np.uint32)


def int_complex(n, amp, seed):
    rng = np.random.default_rng(seed)
    return (rng.integers(-amp, amp + 1, size=n)
            + 1j * rng.integers(-amp, amp + 1, size=n)).astype(np.complex64)


def gauss_complex(shape, seed):
    rng = np.random.default_rng(seed)
    return (rng.normal(size=shape) + 1j * rng.normal(size=shape)
            ).astype(np.complex64)


def power64(x):
    return x.real.astype(np.float64) ** 2 + x.imag.astype(np.float64) ** 2


# ---------------------------------------------------------------------------
# 1. reductions
# ---------------------------------------------------------------------------

@pytest.mark.parametrize(
    "n", [1, 2, 3, 4, 5, 7, 1023]
    + [(1 << 22) + 4 * (1 << 12) + r for r in range(4)])
def test_sum_sumsq_exact(C, n):
    """Integers in [-8, 8]: both sums are integers below 2^53, exact in the
    kernel's fp64 in any order.  n & 3 = 0..3 covers the scalar tail; the
    last four sizes are 2^20 + 2^12 float4s, one more than the 1024 x 256
    threads cover in four trips, so the float4 loop wraps raggedly."""
    rng = np.random.default_rng(n)
    x = rng.integers(-8, 9, size=n).astype(np.float32)
    got = C.sum_sumsq(to_gpu(x)).cpu().numpy()
    x64 = x.astype(np.float64)
    assert got[0] == x64.sum()
    assert got[1] == (x64 * x64).sum()


@pytest.mark.parametrize("n", [1, 2, 3, (1 << 16) + 1, PAST])
def test_mean_power_exact(C, n):
    """Integer re, im in [-7, 7]: a thread's float32 accumulator and every
    fp64 partial are exact integers, and the kernel's last operation is the
    oracle's: float64(sum) / n.  PAST is odd (the scalar tail) and has
    more float4s than the 2^18 threads of pass 1 (the loop wraps)."""
    x = int_complex(n, 7, seed=n)
    want = power64(x).sum() / n
    assert C.mean_power(to_gpu(x)).cpu().numpy()[0] == want


@pytest.mark.parametrize("n,drains", [(3 * (1 << 18) + 1, 1), (1 << 20, 2)])
def test_mean_power_drain(C, n, drains):
    """blocks = 1: 256 threads walk n / 2 float4s, so a thread moves its
    float32 accumulator into the fp64 one every 1024 trips = 2^19 bins.
    3 * 2^18 + 1 bins: 1536 trips, one drain, then half a round, plus the odd
    tail; 2^20 bins: 2048 trips, the second drain on the last trip.  With
    integer amplitudes <= 7 a trip adds at most 196, so the accumulator
    stays below 2^18 between drains and the mean must be exact.  A drain
    that loses `acc` (no `accd += acc`) or counts it twice (no `acc = 0`)
    changes the integer sum, and so does a pass 2 that sums partials pass 1
    never wrote."""
    x = int_complex(n, 7, seed=drains)
    trips = (n // 2) // 256
    assert trips // 1024 == drains
    want = power64(x).sum() / n
    g = to_gpu(x)
    assert C.mean_power(g, blocks=1).cpu().numpy()[0] == want
    # a few blocks: some partials written, the other 1024 - 3 stale
    assert C.mean_power(g, blocks=3).cpu().numpy()[0] == want
    assert C.mean_power(g).cpu().numpy()[0] == want


def test_mean_power_rejects_a_grid_outside_the_partials(C):
    g = to_gpu(int_complex(8, 3, seed=0))
    for blocks in (-1, 1025):
        with pytest.raises(RuntimeError):
            C.mean_power(g, blocks=blocks)


# ---------------------------------------------------------------------------
# 2. standalone spectrum stage
# ---------------------------------------------------------------------------

TIE_THRESHOLD = 9.0


def tie_spectrum(n, seed):
    """Integer bins with mean power exactly 1 = 2^0, for threshold 9: bins
    of power 9 = threshold * mean exactly ((3, 0) and its rotations), of
    power 10 ((3, 1)) one above it, of power 8 ((2, 2)) one below, among
    bins of power 2, 1 and 0.  (n - 1, n, n + 1 are all sums of two squares
    only for odd n, so the mean has to be 1 and the threshold odd.)"""
    t = n // 512                                 # triples of 8 + 9 + 10 = 27
    rest = n - 27 * t                            # power left for the others
    a = rest // 4                                # bins of power 2
    b = rest - 2 * a                             # bins of power 1
    z = n - 3 * t - a - b                        # bins of power 0
    assert t > 0 and z > 0
    rng = np.random.default_rng(seed)

    def rot(re, im, count):
        k = rng.integers(0, 4, size=count)
        return (re + 1j * im) * (1j ** k)

    spec = np.concatenate([rot(2, 2, t), rot(3, 0, t), rot(3, 1, t),
                           rot(1, 1, a), rot(1, 0, b), np.zeros(z)])
    spec = np.round(spec.real) + 1j * np.round(spec.imag) + 0.0
    spec = rng.permutation(spec).astype(np.complex64)
    p = power64(spec)
    assert p.sum() == n
    assert (p == 8).sum() == t and (p == 9).sum() == t and (p == 10).sum() == t
    return spec


def s1_coeff(n, channels):
    """The launcher's float32 normalisation coefficient (n^2 / S)^(-1/2)."""
    return np.float32((float(n) * float(n) / float(channels)) ** -0.5)


@pytest.mark.parametrize("n,channels", [(1 << 12, 1 << 8), (1 << 21, 1 << 10)])
def test_rfi_s1_ties(C, n, channels):
    """threshold * mean = 9 exactly and the comparison is `>`: power 9
    survives (scaled), 10 is zapped, 8 survives.  The coefficient is
    2^-8 / 2^-16, so every survivor is exact and the whole output is compared
    bit for bit.  2^21 bins is past the cap."""
    spec = tie_spectrum(n, seed=n)
    coeff = s1_coeff(n, channels)
    assert np.frexp(coeff)[0] == 0.5             # a power of two
    p = power64(spec)
    zap = p > TIE_THRESHOLD * p.mean()
    assert zap.sum() == (p == 10).sum()
    want = np.where(zap, 0.0, spec.astype(np.complex128) * float(coeff)
                    ).astype(np.complex64)
    g = to_gpu(spec)
    C.rfi_s1(g, TIE_THRESHOLD, channels)
    got = g.cpu().numpy()
    assert (got[p == 9] != 0).all() and (got[p == 10] == 0).all()
    np.testing.assert_array_equal(bits(got), bits(want))
    np.testing.assert_array_equal(
        got, ref.rfi_mitigate_s1(spec, TIE_THRESHOLD, channels))


S1_GAUSS_SEED = 0
S1_GAUSS_THRESHOLD = 4.0


def test_rfi_s1_gaussian_past_cap(C):
    """Against ref.rfi_mitigate_s1 for the decisions, and per survivor
    against float64 v * coeff with the launcher's float32 coefficient: the
    kernel's v * coeff is one rounding, 1 u relative.  The kernel compares a
    float32 power (2 roundings) with a float32 threshold * mean (2 roundings),
    so a bin within 2^-20 = 16 u of the threshold could go either way: the
    seed has none, which is asserted, so no bin is left out."""
    n, channels = PAST, 1 << 8
    spec = gauss_complex(n, S1_GAUSS_SEED)
    spec[[5, CAP - 1, CAP, n - 1]] = 30.0
    p = power64(spec)
    edge = S1_GAUSS_THRESHOLD * p.mean()
    assert np.abs(p / edge - 1.0).min() > 2.0 ** -20
    want = ref.rfi_mitigate_s1(spec, S1_GAUSS_THRESHOLD, channels)
    zap = p > edge
    assert 1000 < zap.sum() < n // 10
    assert ((want == 0) == zap).all()
    g = to_gpu(spec)
    C.rfi_s1(g, S1_GAUSS_THRESHOLD, channels)
    got = g.cpu().numpy()
    np.testing.assert_array_equal(got == 0, zap)
    c = float(s1_coeff(n, channels))
    for part in ("real", "imag"):
        w = getattr(spec, part).astype(np.float64) * c
        err = np.abs(getattr(got, part).astype(np.float64) - w)[~zap]
        r = (err / np.abs(w[~zap])).max() / U
        print(f"rfi_s1 {part}: max err {r:.3f} u")
        assert r <= 1.0


@pytest.mark.parametrize("n,lo,hi", [
    (300, 0, 10), (300, 290, 299), (300, 7, 7), (1, 0, 0),
    (PAST, 1, PAST - 2),      # wider than 2^20: the zero-fill loop wraps
    (PAST, 0, PAST - 1),
])
def test_zap_bins_touches_only_its_range(C, n, lo, hi):
    rng = np.random.default_rng(n + lo)
    spec = (rng.integers(1, 9, size=n) - 1j * rng.integers(1, 9, size=n)
            ).astype(np.complex64)
    want = spec.copy()
    want[lo:hi + 1] = 0
    g = to_gpu(spec)
    C.zap_bins(g, lo, hi)
    np.testing.assert_array_equal(bits(g.cpu().numpy()), bits(want))


def test_zap_bins_rejects_a_range_outside_the_spectrum(C):
    g = to_gpu(np.ones(256, dtype=np.complex64))
    for lo, hi in [(20, 10), (10, 256), (256, 256), (-1, 5), (0, 1 << 40)]:
        with pytest.raises(RuntimeError):
            C.zap_bins(g, lo, hi)
    with pytest.raises(RuntimeError):            # not contiguous
        C.zap_bins(to_gpu(np.ones(512, dtype=np.complex64))[::2], 0, 5)
    with pytest.raises(RuntimeError):            # not complex64
        C.zap_bins(to_gpu(np.ones(256, dtype=np.complex128)), 0, 5)
    assert (g.cpu().numpy() == 1).all()


@pytest.mark.parametrize("dm", [dp.DM, -dp.DM])
def test_phase_table_absolute_error(C, dm):
    """srtb_dedisp_factor on the 2^17-bin band where the turn count is
    largest (~3e6), against the extended-precision oracle of
    test_gpu_dedisp_poly.  The limit is the figure the function's own comment
    promises for its float32 sine and cosine, 1.5e-6 rad; the modulus is
    cos^2 + sin^2 of two results good to ~1 u each, 4 u at most from 1."""
    tab = C.dedisp_phase_table(dp.PH_NC, dp.F_MIN, dp.F_C, dp.PH_DF, dm,
                               torch.device("cuda"))
    err = dp._max_phase_err(tab, dp._oracle(dm))
    mod = np.abs(np.abs(tab.cpu().numpy().astype(np.complex128)) - 1.0).max()
    print(f"per-bin phase, dm {dm}: max wrapped error {err:.3e} rad, "
          f"max | |factor| - 1 | {mod / U:.2f} u")
    assert err <= 1.5e-6
    assert mod <= 4 * U


def test_phase_table_past_cap(C):
    """A table longer than the launch, on the wide band of test_phase_table
    (f_min 1000, bandwidth 500 MHz), at 64 sampled bins and the last one
    against exact rationals: an index that wraps wrongly at i >= 2^20 is an
    error of order 1 rad.  Here |k| reaches 2.2e8 turns, so the fp64 steps
    before the wrap show: f = f_min + df i is 2 roundings, each amplified
    |2 f / (f - f_c) - 1| <= 5 times in k; f - f_c is exact (Sterbenz); the
    division by f_c counts twice (r is squared); r * r, * dm, / f and the
    last product one each: at most 16 roundings of 2^-53 relative, that is
    2 pi * 16 * 2^-53 * |k| rad, plus the 1.5e-6 rad pinned above."""
    n = PAST
    f_min, bw, dm = 1000.0, 500.0, 478.8
    f_c, df = f_min + bw, bw / n
    tab = C.dedisp_phase_table(n, f_min, f_c, df, dm,
                               torch.device("cuda")).cpu().numpy()
    assert tab.shape == (n,)
    worst = 0.0
    for i in sorted(set(range(0, n, n // 63)) | {CAP - 1, CAP, CAP + 1, n - 1}):
        frac = dp._turns_frac_exact(i, f_min, f_c, df, dm)
        f = f_min + df * i
        k = dp.D_MHZ * 1e6 * dm / f * ((f - f_c) / f_c) ** 2
        limit = 2 * np.pi * 16 * 2.0 ** -53 * abs(k) + 1.5e-6
        e = abs(np.angle(complex(tab[i]) * np.exp(2j * np.pi * frac)))
        worst = max(worst, e / limit)
        assert e <= limit, (i, e, limit)
    print(f"phase table past the cap: worst error / limit {worst:.3f}")


# A band on which f = f_min + df i is exact in fp64 whether or not the
# compiler contracts it (dyadic df, 64 MHz over 2^20 bins), so every kernel
# that inlines srtb_dedisp_factor gets the table's bits.
DD_F_MIN, DD_F_C, DD_DF, DD_DM = 1437.0, 1437.0 - 64.0, -(2.0 ** -14), -478.8


def dd_table(C, n):
    return C.dedisp_phase_table(n, DD_F_MIN, DD_F_C, DD_DF, DD_DM,
                                torch.device("cuda"))


def assert_rotated(got, v, coeff, table, zap, what):
    """got = v * coeff * table[i] to 3 u |v coeff| per component where not
    zapped, exactly 0 where zapped."""
    t = table.astype(np.complex128)
    want = v.astype(np.complex128) * float(coeff) * t
    limit = 3 * U * np.abs(v.astype(np.complex128)) * float(coeff)
    got = got.astype(np.complex128)
    assert (got[zap] == 0).all(), what
    keep = ~zap
    assert keep.sum() > got.size // 2
    worst = 0.0
    for part in (np.real, np.imag):
        e = np.abs(part(got) - part(want))[keep]
        assert (e <= limit[keep]).all(), (what, part.__name__)
        nz = limit[keep] > 0
        worst = max(worst, (e[nz] / limit[keep][nz]).max())
    print(f"{what}: worst error / limit {worst:.3f}")


def test_dedisperse_in_place_past_cap(C):
    """The expected output comes from the table the GPU just produced (its
    phase is bounded above), in float64: what is left is the complex
    multiply, a rounded product and an fma or two products and a sum per
    component, 2 u (|v.x t.x| + |v.y t.y|) <= 2 u |v| |t| < 3 u |v|."""
    n = PAST
    spec = gauss_complex(n, seed=31)
    table = dd_table(C, n).cpu().numpy()
    g = to_gpu(spec)
    C.dedisperse(g, DD_F_MIN, DD_F_C, DD_DF, DD_DM)
    assert_rotated(g.cpu().numpy(), spec, 1.0, table,
                   np.zeros(n, dtype=bool), "dedisperse")


def fused_ranges(n):
    """16 ranges: two overlapping, single bins, one across the 2^20 wrap, one
    ending at n - 1, one starting past n (harmless: i < n guards it)."""
    r = [[100, 300], [250, 400], [0, 0], [777, 777], [CAP - 5, CAP + 5],
         [n - 9, n - 1], [n + 5, n + 100], [5000, 4000]]
    r += [[10000 * k, 10000 * k + k] for k in range(1, 9)]
    assert len(r) == 16
    return r


def range_mask(n, ranges):
    m = np.zeros(n, dtype=bool)
    for lo, hi in ranges:
        m[lo:hi + 1] = True       # empty for hi < lo, clipped past n
    return m


@pytest.mark.parametrize("use_table", [False, True])
def test_fused_in_place_past_cap_no_rfi(C, use_table):
    """Manual zaps and the rotation only; 3 u |v| as for dedisperse (the
    fused kernel's multiply is a rounded product and an fma)."""
    n = PAST
    spec = gauss_complex(n, seed=32)
    tab = dd_table(C, n)
    ranges = fused_ranges(n)
    g = to_gpu(spec)
    C.rfi_dedisperse_fused(g, False, 0.0, 1, ranges, DD_F_MIN, DD_F_C, DD_DF,
                           DD_DM, tab if use_table else None)
    assert_rotated(g.cpu().numpy(), spec, 1.0, tab.cpu().numpy(),
                   range_mask(n, ranges), f"fused, table={use_table}")


@pytest.mark.parametrize("use_table", [False, True])
def test_fused_in_place_past_cap_rfi_ties(C, use_table):
    """The tie spectrum of test_rfi_s1_ties at 2^21 bins: power 9 = threshold
    * mean survives, 10 is zapped, and so is every bin of the 16 ranges.  The
    coefficient is 2^-16, exact, so 3 u |v coeff| bounds the multiply alone."""
    n, channels = 1 << 21, 1 << 10
    spec = tie_spectrum(n, seed=n)
    coeff = s1_coeff(n, channels)
    tab = dd_table(C, n)
    ranges = fused_ranges(n)
    p = power64(spec)
    ranged = range_mask(n, ranges)
    zap = (p > TIE_THRESHOLD * p.mean()) | ranged
    assert ((p == 9) & ~ranged).sum() > 1000 and ((p == 10) & ~ranged).any()
    g = to_gpu(spec)
    C.rfi_dedisperse_fused(g, True, TIE_THRESHOLD, channels, ranges, DD_F_MIN,
                           DD_F_C, DD_DF, DD_DM, tab if use_table else None)
    got = g.cpu().numpy()
    assert (got[(p == 9) & ~ranged] != 0).all()
    assert_rotated(got, spec, coeff, tab.cpu().numpy(), zap,
                   f"fused with RFI, table={use_table}")


def test_fused_rejects_17_ranges_and_a_short_table(C):
    g = to_gpu(gauss_complex(64, seed=1))
    before = g.cpu().numpy().copy()
    with pytest.raises(RuntimeError):
        C.rfi_dedisperse_fused(g, False, 0.0, 1, [[k, k] for k in range(17)],
                               DD_F_MIN, DD_F_C, DD_DF, DD_DM)
    with pytest.raises(RuntimeError):
        C.rfi_dedisperse_fused(g, False, 0.0, 1, [], DD_F_MIN, DD_F_C, DD_DF,
                               DD_DM, dd_table(C, 63))
    np.testing.assert_array_equal(bits(g.cpu().numpy()), bits(before))


# ---------------------------------------------------------------------------
# 3. SK method 1
# ---------------------------------------------------------------------------

def sk_v1_int_waterfall(M, nbins, seed):
    """Column j is of kind j % 4: integer noise of amplitude <= 3, constant
    modulus 5 (SK = 1), all zero, a single spike."""
    rng = np.random.default_rng(seed)
    wf = (rng.integers(-3, 4, size=(M, nbins))
          + 1j * rng.integers(-3, 4, size=(M, nbins)))
    j = np.arange(nbins)
    rot = (1 + 2j) * 1j ** rng.integers(0, 4, size=(M, nbins))
    wf[:, j % 4 == 1] = rot[:, j % 4 == 1]
    wf[:, j % 4 == 2] = 0
    spike = j % 4 == 3
    wf[:, spike] = 0
    wf[rng.integers(0, M, size=int(spike.sum())), j[spike]] = 3 - 2j
    wf = np.round(wf.real) + 1j * np.round(wf.imag) + 0.0
    return wf.astype(np.complex64)


@pytest.mark.parametrize("M,nbins", [
    (256, 96), (1, 5), (37, 1), (64, 257),
    (4100, 257),        # M * bins past the cap: the zap loop wraps
    (2, CAP + 5),       # more bins than 2^20: one thread per bin, every bin
])
def test_sk_v1_stats_exact(C, M, nbins):
    """Integer amplitudes <= 3: |x|^2 <= 18, |x|^4 <= 324, and over M <= 4100
    samples s4 <= 1.4e6 < 2^24, so the float32 column sums are exact."""
    wf = sk_v1_int_waterfall(M, nbins, seed=M + nbins)
    p = power64(wf)
    s2, s4 = p.sum(axis=0), (p * p).sum(axis=0)
    assert s4.max() < 2 ** 24
    got = C.sk_v1_mitigate(to_gpu(wf), 1.05, False).cpu().numpy()
    assert got.shape == (nbins, 2) and got.dtype == np.float32
    np.testing.assert_array_equal(got[:, 0], s2)
    np.testing.assert_array_equal(got[:, 1], s4)


# (threshold, seed) per shape: both decisions occur among the Gaussian
# columns, and the seed keeps every column's SK clear of the thresholds
SK_V1_CASE = {(256, 96): (1.1, 1), (4100, 257): (1.05, 2)}


def sk_v1_decisions(wf, threshold):
    """(zap, relative distance of SK to the nearer corrected threshold)."""
    M = wf.shape[0]
    hi, lo = threshold, 2.0 - threshold
    corr = (M - 1.0) / (M + 1.0)
    lo_, hi_ = lo * corr + 1.0, hi * corr + 1.0
    p = power64(wf)
    s2, s4 = p.sum(axis=0), (p * p).sum(axis=0)
    with np.errstate(divide="ignore", invalid="ignore"):
        sk = M * s4 / (s2 * s2)
    zap = (sk > hi_) | (sk < lo_) | (s2 == 0)
    with np.errstate(invalid="ignore"):
        margin = np.minimum(np.abs(sk / lo_ - 1.0), np.abs(sk / hi_ - 1.0))
    return zap, np.where(s2 == 0, np.inf, margin)


@pytest.mark.parametrize("normalize", [False, True])
@pytest.mark.parametrize("M,nbins", [(256, 96), (4100, 257)])
def test_sk_v1_zap_decision(C, M, nbins, normalize):
    """The kernel forms SK from float32 column sums, so a column whose
    float64 SK lies within 1e-5 relative of a corrected threshold could go
    either way: the seed has none (asserted), no column is left out.
    Without normalize a kept column is the input bit for bit and a zapped one
    is zero.  With normalize a kept element is x * rsqrt(s2 / M) with the
    float32 s2 the call returns (pinned exactly above): the division is one
    rounding, halved by the root (0.5 u), the hardware reciprocal square root
    is good to 1 ulp = 2 u, the multiply 1 u: 4 u covers them."""
    threshold, seed = SK_V1_CASE[(M, nbins)]
    wf = gauss_complex((M, nbins), seed)
    wf[:, 3] = (1 + 2j)                   # constant modulus: SK = 1, zapped
    wf[:, 4] = 0                          # no power: zapped
    wf[:, 5] = 0
    wf[::40, 5] = 25.0                    # spikes: SK = 40, zapped
    zap, margin = sk_v1_decisions(wf, threshold)
    assert margin.min() > 1e-5
    assert zap[3] and zap[4] and zap[5]
    assert zap.sum() > 10 and (~zap).sum() > nbins // 4
    np.testing.assert_array_equal(
        np.abs(ref.rfi_mitigate_sk_v1(wf, threshold)).sum(axis=0) == 0,
        zap)
    g = to_gpu(wf)
    s2 = C.sk_v1_mitigate(g, threshold, normalize).cpu().numpy()[:, 0]
    got = g.cpu().numpy()
    assert (got[:, zap] == 0).all()
    if not normalize:
        np.testing.assert_array_equal(bits(got[:, ~zap]), bits(wf[:, ~zap]))
        return
    scale = 1.0 / np.sqrt(s2[~zap].astype(np.float64) / M)
    worst = 0.0
    for part in ("real", "imag"):
        w = getattr(wf, part)[:, ~zap].astype(np.float64) * scale[None, :]
        e = np.abs(getattr(got, part)[:, ~zap].astype(np.float64) - w)
        worst = max(worst, (e / np.abs(w)).max() / U)
    print(f"sk_v1 normalize M {M}: max err {worst:.3f} u")
    assert worst <= 4.0


# ---------------------------------------------------------------------------
# 4. running_mean
# ---------------------------------------------------------------------------

def running_mean_stepped(data, w, dtype):
    """ref.running_mean's recurrence over all channels at once, the initial
    average (a sequential sum / w) included, stepped in `dtype`.  Returns
    (out, ave, |head - a| at every output)."""
    x = np.asarray(data, dtype=dtype)
    nsamp, nchan = x.shape
    wd = dtype(w)
    a = np.zeros(nchan, dtype=dtype)
    for k in range(w):
        a = a + x[k]
    a = a / wd
    out = np.zeros((nsamp, nchan), dtype=np.uint8)
    gap = np.zeros((nsamp, nchan), dtype=np.float64)
    for i in range(w, nsamp):
        head, tail = x[i - w], x[i]
        out[i - w] = head > a
        gap[i - w] = np.abs(head.astype(np.float64) - a)
        a = a + (tail - head) / wd
    for i in range(w):
        head, tail = x[nsamp + i - w], x[nsamp - i - 1]
        out[i + nsamp - w] = head > a
        gap[i + nsamp - w] = np.abs(head.astype(np.float64) - a)
        a = a + (tail - head) / wd
    assert a.dtype == dtype
    return out, a, gap


@pytest.mark.parametrize("nsamp,nchan,w", [
    (64, 300, 16),      # crosses a workgroup
    (16, 3, 16),        # only the mirrored tail
    (17, 5, 16), (40, 2, 1), (4096, 1, 64),
    (2, CAP + 3, 1),    # more channels than 2^20: one thread each, every one
])
def test_running_mean_exact(C, nsamp, nchan, w):
    """Integers in [-8, 8] and a power-of-two window: the mean is a multiple
    of 1 / w below 8 and every update is exact in float32, so `out` and `ave`
    equal the float64 oracle's, at samples equal to the running mean too
    (`>` must give 0 there; the count of such samples is asserted > 0)."""
    rng = np.random.default_rng(1)
    data = rng.integers(-8, 9, size=(nsamp, nchan)).astype(np.float32)
    eout, eave, gap = running_mean_stepped(data, w, np.float64)
    if nchan <= 300:    # the stepped oracle is ref.running_mean
        rout, rave = ref.running_mean(
            data, w, ref.running_mean_init_average(data, w))
        np.testing.assert_array_equal(rout, eout)
        np.testing.assert_array_equal(rave, eave)
    ties = int((gap == 0).sum())
    print(f"running_mean {(nsamp, nchan, w)}: {ties} samples equal the mean")
    if (nsamp, nchan, w) in [(64, 300, 16), (2, CAP + 3, 1)]:
        assert ties > 0
    out, ave = C.running_mean(to_gpu(data), w)
    np.testing.assert_array_equal(out.cpu().numpy(), eout)
    np.testing.assert_array_equal(ave.cpu().numpy(), eave)


def test_running_mean_window_12(C):
    """A window that is no power of two, Gaussian data about 10: the oracle
    for the bits is the same recurrence stepped in float32 (subtract, divide,
    add: correctly rounded operations, nothing to contract).  Should the
    kernel round an update otherwise, a bit may differ only where |head - a|
    in float64 is below 8 u max|data|; at most 0.5 % of the outputs may lie
    there (asserted; the seed has none).  `ave`: 100 updates of at most
    u |a| + 2 u |tail - head| / 12 each, below 1.05 u |a|: 1e-5 relative."""
    nsamp, nchan, w = 100, 70, 12
    rng = np.random.default_rng(2)
    data = (10.0 + rng.normal(size=(nsamp, nchan))).astype(np.float32)
    out32, ave32, _ = running_mean_stepped(data, w, np.float32)
    out64, ave64, gap = running_mean_stepped(data, w, np.float64)
    near = gap < 8 * U * np.abs(data).max()
    assert near.sum() <= 0.005 * near.size
    assert ((out32 != out64) & ~near).sum() == 0
    out, ave = C.running_mean(to_gpu(data), w)
    out, ave = out.cpu().numpy(), ave.cpu().numpy()
    differ = out != out32
    print(f"running_mean window 12: {int(near.sum())} samples near the mean, "
          f"{int(differ.sum())} bits differ from the float32 recurrence")
    assert (differ & ~near).sum() == 0
    np.testing.assert_allclose(ave, ave64, rtol=1e-5, atol=0)


def test_running_mean_rejects_a_window_outside_the_data(C):
    g = to_gpu(np.ones((8, 4), dtype=np.float32))
    for w in (0, 9, -1):
        with pytest.raises(RuntimeError):
            C.running_mean(g, w)
    out, _ = C.running_mean(g, 8)
    assert out.shape == (8, 4)


# ---------------------------------------------------------------------------
# 5. display
# ---------------------------------------------------------------------------

RESAMPLE_SHAPES = [
    (64, 256, 16, 32),          # integer ratios
    (8, 130, 8, 130),           # one to one
    (37, 301, 7, 13),           # fractional both ways
    (5, 1000, 16, 3),           # upsampling in y, 334 columns per pixel in x
    (3, 5, 8, 16),              # output cells inside one source cell
    (1, 64, 1, 1),
    (70, 700, 1, 1),            # 11 trips with a ragged last one, 70 rows
    (2, CAP + 6, 2, 3),         # a row longer than 2^20
]


def resample_chain(rows, length, H, W):
    """T: the longest chain of additions in one lane, ceil(columns covered /
    64) * rows covered, over the output pixels."""
    def covered(n_in, n_out):
        s = n_in / n_out
        return max(min(int(np.ceil((o + 1) * s)), n_in) - int(np.floor(o * s))
                   for o in range(n_out))
    return -(-covered(length, W) // 64) * covered(rows, H)


_resample_ratio = {}


@pytest.mark.parametrize("rows,length,H,W", RESAMPLE_SHAPES)
def test_resample_power(C, rows, length, H, W):
    """Against ref.resample_power_2d of the float64 power.  Every term
    wy * wx * |x|^2 is non-negative, so relative errors do not amplify: a
    pixel is off by at most (T + 16) u relative, T = the length of a lane's
    addition chain (one rounding per addition) and 16 for what every term
    and the result go through besides: the two weights (1 each), their
    product (1), the power (3: two products and a sum, or 2 contracted), the
    product with it (1), the six shuffle steps of the wave reduction (6), the
    area's rounding (1) and the division (1): 15, rounded up."""
    wf = gauss_complex((rows, length), seed=rows + length)
    got = C.resample_power(to_gpu(wf), H, W).cpu().numpy()
    assert got.shape == (H, W) and got.dtype == np.float32
    want = ref.resample_power_2d(power64(wf), H, W)
    assert (want > 0).all()
    bound = (resample_chain(rows, length, H, W) + 16) * U
    ratio = (np.abs(got - want) / want).max() / bound
    _resample_ratio[(rows, length, H, W)] = ratio
    print(f"resample {(rows, length, H, W)}: max err / bound {ratio:.4f}")
    assert ratio <= 1.0


@pytest.mark.parametrize("rows,length,H,W", RESAMPLE_SHAPES[:2])
def test_resample_power_exact(C, rows, length, H, W):
    """Integer ratios: every weight is 1, the area a power of two (or 1) and
    the terms small integers, so the average is exact."""
    wf = int_complex(rows * length, 5, seed=length).reshape(rows, length)
    got = C.resample_power(to_gpu(wf), H, W).cpu().numpy()
    want = ref.resample_power_2d(power64(wf), H, W)
    np.testing.assert_array_equal(got, want)


@pytest.mark.parametrize("rows,length,H,W", [(3, 5, 8, 16), (5, 1000, 16, 3)])
def test_resample_power_constant_image(C, rows, length, H, W):
    """|x|^2 = 25 everywhere: the sum of the weights over the area must give
    25 back to 4 u.  Shapes whose cells lie inside one or two source cells in
    one direction at least, where nothing but the weights' own roundings
    enters: a weight that is wrong at an edge (the clamp, the fractional
    coverage) is an error of order 1 / cells covered."""
    wf = np.full((rows, length), 3 - 4j, dtype=np.complex64)
    got = C.resample_power(to_gpu(wf), H, W).cpu().numpy().astype(np.float64)
    worst = np.abs(got / 25.0 - 1.0).max() / U
    print(f"resample constant {(rows, length, H, W)}: max err {worst:.2f} u")
    assert worst <= 4.0


def test_resample_power_rejects_an_empty_image(C):
    g = to_gpu(gauss_complex((4, 8), seed=0))
    for H, W in [(0, 4), (4, 0), (-1, 4), (4, -2)]:
        with pytest.raises(RuntimeError):
            C.resample_power(g, H, W)
    with pytest.raises(RuntimeError):
        C.resample_power(to_gpu(np.zeros((0, 8), dtype=np.complex64)), 2, 2)


def mean_two_image(n, seed):
    """Integers in 0..4 whose mean is exactly 2: pairs 2 - k, 2 + k."""
    rng = np.random.default_rng(seed)
    k = rng.integers(0, 3, size=n // 2)
    img = np.concatenate([2 - k, 2 + k, [2] * (n & 1)])
    return rng.permutation(img).astype(np.float32)


@pytest.mark.parametrize("n", [1, 3, 1000, PAST])
def test_normalize_by_mean_exact(C, n):
    """Mean 2 exactly: the scale 1 / (2 mean) = 1 / 4 and every product are
    exact."""
    img = mean_two_image(n, seed=n)
    assert img.astype(np.float64).mean() == 2.0
    g = to_gpu(img)
    C.normalize_by_mean(g)
    np.testing.assert_array_equal(bits(g.cpu().numpy()), bits(img / 4))
    np.testing.assert_array_equal(g.cpu().numpy(), ref.normalize_by_mean(img))


def test_normalize_by_mean_leaves_a_zero_image(C):
    g = to_gpu(np.zeros(1000, dtype=np.float32))
    C.normalize_by_mean(g)
    np.testing.assert_array_equal(bits(g.cpu().numpy()),
                                  np.zeros(1000, dtype=np.uint32))


# second colour pair: alpha and red descend (c0 > c1), green and blue ascend
COLOR_PAIRS = [
    (ref.COLOR_0, ref.COLOR_1, ref.COLOR_OVERFLOW),
    (0xFFF0207F, 0x00103080, 0x12345678),
]


def pixmap_oracle(x, c0, c1, cover, tolerant=False):
    """The rule of srtb_kernels.h in float64: nearest, ties away from zero,
    of a + (b - a) x per channel; 0 <= x <= 1 or the overflow colour.  With
    tolerant=True also returns, per pixel, whether some channel's exact value
    is within 2^-16 of a half-integer."""
    x = np.asarray(x, dtype=np.float64)
    ok = (x >= 0) & (x <= 1)
    xs = np.where(ok, x, 0.0)
    out = np.zeros(x.shape, dtype=np.uint32)
    band = np.zeros(x.shape, dtype=bool)
    for sh in (0, 8, 16, 24):
        a, b = float((c0 >> sh) & 0xFF), float((c1 >> sh) & 0xFF)
        v = a + (b - a) * xs
        out |= np.floor(v + 0.5).astype(np.uint32) << np.uint32(sh)
        band |= np.abs(v - np.floor(v) - 0.5) <= 2.0 ** -16
    out[~ok] = cover
    return (out, band & ok) if tolerant else out


def gpu_pixmap(C, x, c0, c1, cover):
    pix = C.generate_pixmap(to_gpu(x), c0, c1, cover).cpu().numpy()
    return pix.view(np.uint32)


PIXMAP_GRID = (np.arange(4097, dtype=np.float64) / 4096).astype(np.float32)


@pytest.mark.parametrize("c0,c1,cover", COLOR_PAIRS)
def test_generate_pixmap_grid(C, c0, c1, cover):
    """x = j / 4096: (b - a) x has at most 8 + 13 bits and a + (b - a) x at
    most 8 + 12, so the float32 value is exact, contracted or not, and every
    pixel must match, the GUI colours' three ties (0.25, 0.375, 0.875)
    included."""
    want = pixmap_oracle(PIXMAP_GRID, c0, c1, cover)
    if c0 == ref.COLOR_0:
        np.testing.assert_array_equal(want, ref.generate_pixmap(PIXMAP_GRID))
        j = [1024, 1536, 3584]
        assert [hex(v) for v in want[j]] == ["0xff244f63", "0xff27677a",
                                             "0xff31c9d9"]
    np.testing.assert_array_equal(gpu_pixmap(C, PIXMAP_GRID, c0, c1, cover),
                                  want)


@pytest.mark.parametrize("c0,c1,cover", COLOR_PAIRS)
def test_generate_pixmap_edges(C, c0, c1, cover):
    """0 <= x <= 1 at its ends.  -0.0 is in range.  The smallest negative
    subnormal is below 0: the build keeps float32 subnormals (observed on
    MI355X: it takes the overflow colour, as in the oracle)."""
    one = np.float32(1.0)
    x = np.array([0.0, -0.0, 1.0, np.nextafter(one, np.float32(2.0)),
                  -np.float32(1e-45), np.nan, np.inf, -np.inf,
                  np.float32(1e-45), -np.float32(2.0 ** -126)],
                 dtype=np.float32)
    assert x[4] < 0 and x[4] == -2.0 ** -149
    want = np.array([c0, c0, c1, cover, cover, cover, cover, cover, c0,
                     cover], dtype=np.uint32)
    np.testing.assert_array_equal(pixmap_oracle(x, c0, c1, cover), want)
    got = gpu_pixmap(C, x, c0, c1, cover)
    print("pixmap of the smallest negative subnormal:",
          "overflow (subnormals kept)" if got[4] == cover else hex(got[4]))
    np.testing.assert_array_equal(got, want)


@pytest.mark.parametrize("c0,c1,cover", COLOR_PAIRS)
def test_generate_pixmap_random(C, c0, c1, cover):
    """200 000 uniform float32 in [0, 1).  The kernel evaluates a + (b - a) x
    in float32: the product and the sum are each below 256, where half an
    ulp is 2^-17, so the two roundings (one if contracted) move the value by
    2^-16 at most.  Where the exact value is within 2^-16 of a half-integer
    either neighbour passes; everywhere else the channel must match.  At most
    0.1 % of the inputs may lie in that band (asserted)."""
    rng = np.random.default_rng(0)
    x = rng.random(200_000, dtype=np.float32)
    want, band = pixmap_oracle(x, c0, c1, cover, tolerant=True)
    assert band.sum() <= 0.001 * x.size
    got = gpu_pixmap(C, x, c0, c1, cover)
    np.testing.assert_array_equal(got[~band], want[~band])
    for sh in (0, 8, 16, 24):
        d = (((got[band] >> sh) & 0xFF).astype(np.int64)
             - ((want[band] >> sh) & 0xFF).astype(np.int64))
        assert (np.abs(d) <= 1).all()
    print(f"pixmap random: {int(band.sum())} inputs in the band, "
          f"{int((got != want).sum())} differ")


def test_generate_pixmap_past_cap(C):
    c0, c1, cover = COLOR_PAIRS[0]
    x = np.resize(np.concatenate([PIXMAP_GRID, [-1.0, 2.0, np.nan]]
                                 ).astype(np.float32), PAST)
    np.testing.assert_array_equal(gpu_pixmap(C, x, c0, c1, cover),
                                  pixmap_oracle(x, c0, c1, cover))


def test_generate_pixmap_rejects_what_it_cannot_index(C):
    c0, c1, cover = COLOR_PAIRS[0]
    with pytest.raises(RuntimeError):            # not contiguous
        C.generate_pixmap(to_gpu(PIXMAP_GRID)[::2], c0, c1, cover)
    with pytest.raises(RuntimeError):            # not float32
        C.generate_pixmap(to_gpu(PIXMAP_GRID.astype(np.float64)), c0, c1,
                          cover)


# ---------------------------------------------------------------------------
# 6. correlator
# ---------------------------------------------------------------------------

CORR_SCALE = 3.0 * 2.0 ** -10    # exact in float32


def test_correlate_past_cap_plain_and_aliased(C):
    """corr = scale * f1 * conj(f2).  Per component two products and a sum
    (a rounded product and an fma when contracted), then the scale: 3 u of
    (|a.x b.x| + |a.y b.y|) scale for the real part, of (|a.y b.x| +
    |a.x b.y|) scale for the imaginary one.  mag = sqrt(c.x^2 + c.y^2) of
    the float32 corr: the sum is off by 2 u at most, 1 u after the root, plus
    the root's rounding: 2 u.  out = f1 is what srtb-correlator does; it must
    give the plain call's bits."""
    n = PAST
    f1, f2 = gauss_complex(n, seed=41), gauss_complex(n, seed=42)
    g1, g2 = to_gpu(f1), to_gpu(f2)
    corr, mag = C.correlate(g1, g2, CORR_SCALE)
    corr, mag = corr.cpu().numpy(), mag.cpu().numpy()
    np.testing.assert_array_equal(bits(g1.cpu().numpy()), bits(f1))
    ax, ay = f1.real.astype(np.float64), f1.imag.astype(np.float64)
    bx, by = f2.real.astype(np.float64), f2.imag.astype(np.float64)
    for got, want, size in [
            (corr.real, CORR_SCALE * (ax * bx + ay * by),
             CORR_SCALE * (np.abs(ax * bx) + np.abs(ay * by))),
            (corr.imag, CORR_SCALE * (ay * bx - ax * by),
             CORR_SCALE * (np.abs(ay * bx) + np.abs(ax * by)))]:
        r = (np.abs(got.astype(np.float64) - want) / (3 * U * size)).max()
        print(f"correlate: worst error / limit {r:.3f}")
        assert r <= 1.0
    np.testing.assert_allclose(corr, ref.correlate_spectra(f1, f2, CORR_SCALE),
                               rtol=0, atol=1e-6)
    want_mag = np.abs(corr.astype(np.complex128))
    r = (np.abs(mag.astype(np.float64) - want_mag) / want_mag).max() / U
    print(f"correlate mag: max err {r:.3f} u")
    assert r <= 2.0
    # out = f1, exactly aliased
    corr2, mag2 = C.correlate(g1, g2, CORR_SCALE, out=g1)
    assert corr2.data_ptr() == g1.data_ptr()
    np.testing.assert_array_equal(bits(g1.cpu().numpy()), bits(corr))
    np.testing.assert_array_equal(bits(mag2.cpu().numpy()), bits(mag))
    np.testing.assert_array_equal(bits(g2.cpu().numpy()), bits(f2))
    # out = f2
    g1 = to_gpu(f1)
    C.correlate(g1, g2, CORR_SCALE, out=g2)
    np.testing.assert_array_equal(bits(g2.cpu().numpy()), bits(corr))


def test_correlate_rejects_mismatched_inputs(C):
    n = 512
    g1 = to_gpu(gauss_complex(n, seed=1))
    with pytest.raises(RuntimeError):            # f2 shorter than f1
        C.correlate(g1, to_gpu(gauss_complex(n - 1, seed=2)), 1.0)
    with pytest.raises(RuntimeError):            # another dtype
        C.correlate(g1, to_gpu(gauss_complex(n, seed=2).astype(np.complex128)),
                    1.0)
    with pytest.raises(RuntimeError):            # not contiguous
        C.correlate(g1, to_gpu(gauss_complex(2 * n, seed=2))[::2], 1.0)
    with pytest.raises(RuntimeError):            # out of another size
        C.correlate(g1, g1, 1.0, out=to_gpu(gauss_complex(n + 1, seed=3)))
    big = to_gpu(gauss_complex(n + 8, seed=4))
    with pytest.raises(RuntimeError):            # out overlaps f1 partly
        C.correlate(big[:n], big[8:], 1.0, out=big[8:])


def test_complex_abs(C):
    """sqrt(x^2 + y^2) in float32: 2 u as for correlate's mag; 0 at 0."""
    x = gauss_complex(PAST, seed=43)
    x[[0, CAP, PAST - 1]] = 0
    x[1] = 3 + 4j
    mag = C.complex_abs(to_gpu(x)).cpu().numpy()
    assert mag.dtype == np.float32 and mag.shape == (PAST,)
    assert mag[0] == 0 and mag[CAP] == 0 and mag[-1] == 0 and mag[1] == 5
    want = np.abs(x.astype(np.complex128))
    nz = want > 0
    r = (np.abs(mag[nz].astype(np.float64) - want[nz]) / want[nz]).max() / U
    print(f"complex_abs: max err {r:.3f} u")
    assert r <= 2.0
    with pytest.raises(RuntimeError):
        C.complex_abs(to_gpu(x.astype(np.complex128)))
