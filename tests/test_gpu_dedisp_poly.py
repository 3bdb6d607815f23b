"""GPU tests: column-polynomial dedispersion phase of the backward FFT's
fused pre-op (csrc/kernels/common.h srtb_dedisp_poly_*), against the per-bin
fp64 formula it replaces (srtb_dedisp_factor, reachable through
dedisp_phase_table / rfi_dedisperse_fused and through SRTB_DEDISP_POLY=0).

Measured on MI355X (see profiles/dedisp_poly_kernel_stats.md): max wrapped
phase error 1.7-1.9e-7 rad for the polynomial against 7.0e-7 rad for the
per-bin formula, on the same bins.
"""

from fractions import Fraction

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

# J1644-4559 flagship configuration (bench.py): 1437 MHz top edge, -64 MHz
F_MIN = 1437.0
F_C = 1437.0 - 64.0
DM = -478.80
D_MHZ = 4.148808e3  # kDispersionConstantMHz


@pytest.fixture(scope="module")
def C():
    from srtb_amd.ops import native
    torch.cuda.set_device(0)
    return native()


# ---------------------------------------------------------------- phase ----

# The flagship's first backward pass has N = 64, stride 2^12 at
# df = -64/2^29 MHz: delta = df * stride = -2^-11 MHz per column step.  The
# same delta on 2^17 bins: stride 16, df = -2^-15 MHz (a 4 MHz band starting
# at f_min, where the turn count is largest, ~3e6).
PH_NC = 1 << 17
PH_STRIDE = 16
PH_DF = -(2.0 ** -11) / PH_STRIDE


def _turns_frac_longdouble(nc, f_min, f_c, df, dm):
    """frac(k) per bin, k = D*1e6*dm/f*((f-f_c)/f_c)^2, in extended precision.

    f is exact (dyadic df); the few 2^-64 relative roundings that follow
    leave ~1e-12 turns at |k| ~ 3e6."""
    ld = np.longdouble
    assert np.finfo(ld).nmant >= 63, "needs 80-bit long double"
    f = ld(f_min) + ld(df) * np.arange(nc, dtype=ld)
    r = (f - ld(f_c)) / ld(f_c)
    k = ld(D_MHZ * 1e6) * ld(dm) / f * (r * r)
    return (k - np.floor(k)).astype(np.float64)


def _turns_frac_exact(i, f_min, f_c, df, dm):
    f = Fraction(f_min) + Fraction(df) * i
    r = (f - Fraction(f_c)) / Fraction(f_c)
    k = Fraction(D_MHZ * 1e6) * Fraction(dm) / f * r * r
    return float(k - (k.numerator // k.denominator))


_oracle_cache = {}


def _oracle(dm):
    if dm not in _oracle_cache:
        fr = _turns_frac_longdouble(PH_NC, F_MIN, F_C, PH_DF, dm)
        # the extended-precision oracle itself, against exact rationals
        for i in list(range(0, PH_NC, PH_NC // 64)) + [PH_NC - 1]:
            ex = _turns_frac_exact(i, F_MIN, F_C, PH_DF, dm)
            d = abs(fr[i] - ex)
            assert min(d, 1.0 - d) < 1e-11
        fr.setflags(write=False)
        _oracle_cache[dm] = fr
    return _oracle_cache[dm]


def _max_phase_err(factors, frac_turns):
    """max |arg(factor * exp(+2 pi i frac(k)))|: the factor is exp(-2 pi i k)"""
    z = factors.cpu().numpy().astype(np.complex128)
    return float(np.abs(np.angle(z * np.exp(2j * np.pi * frac_turns))).max())


_table_err_cache = {}


def _table_err(C, dm):
    if dm not in _table_err_cache:
        tab = C.dedisp_phase_table(PH_NC, F_MIN, F_C, PH_DF, dm,
                                   torch.device("cuda"))
        _table_err_cache[dm] = _max_phase_err(tab, _oracle(dm))
    return _table_err_cache[dm]


@pytest.mark.parametrize("dm", [DM, -DM])
@pytest.mark.parametrize("n", [64, 32, 16])
def test_poly_phase_not_worse_than_fp64_formula(C, n, dm):
    got = C.dedisp_poly_factors(PH_NC, n, PH_STRIDE, F_MIN, F_C, PH_DF, dm,
                                torch.device("cuda"))
    e_poly = _max_phase_err(got, _oracle(dm))
    e_tab = _table_err(C, dm)
    print(f"phase err N={n} dm={dm}: poly {e_poly:.3e} rad, "
          f"per-bin fp64 formula {e_tab:.3e} rad")
    assert e_poly <= e_tab


# ----------------------------------------------------------- end to end ----

BATCH = 8
# zap ranges: one straddling a column of every plan below (a column is
# strided, so any run shorter than the stride hits part of many columns and
# a longer one hits several elements of some), one crossing a row boundary
def _zaps(length):
    return [[3 * length + 100, 3 * length + 700],
            [5 * length - 50, 5 * length + 300]]


# (len, maxcol_log2, final_log2): first-pass kernel
PLANS = [
    (1 << 14, 0, 8),   # [64] + 256      -> k_fft_col_pair64
    (1 << 14, 5, 8),   # [8, 8] + 256    -> k_fft_col<8>
]
# These two are native_fft's own factorisation of their length, so the
# per-bin path reproduces the unfused reference bit for bit and "twice its
# error" is no tolerance; they are compared with the per-bin path directly.
SAME_AS_DEFAULT_PLANS = [
    (1 << 13, 5, 8),   # [32] + 256      -> k_fft_col_pair32 / k_fft_col<32>
    (1 << 14, 5, 6),   # [16, 16] + 64   -> k_fft_col<16>
]


def _spec(length):
    rng = np.random.default_rng(length)
    x = (rng.normal(size=(BATCH, length)) +
         1j * rng.normal(size=(BATCH, length))).astype(np.complex64)
    return torch.from_numpy(x).cuda()


def _narrow_df(length):
    # one row spans 2^-5 MHz = 31 kHz like a flagship channel
    return -(2.0 ** -5) / length


def _wide_df(length):
    # the full 64 MHz over the 8 rows: a column spans up to 8 MHz
    return -64.0 / (BATCH * length)


def _reference(C, spec, df, dm, rfi):
    g = spec.clone()
    C.rfi_dedisperse_fused(g, rfi, 4.0, BATCH, _zaps(spec.shape[1]), F_MIN,
                           F_C, df, dm)
    return C.native_fft(g, 1)


def _fused(C, spec, plan, df, dms, rfi):
    _, maxcol, final = plan
    return C.preop_backward_fft(spec, maxcol, final, F_MIN, F_C, df, dms,
                                _zaps(spec.shape[1]), rfi, 4.0, BATCH)


def _max_err(out, ref):
    return float((out - ref).abs().max() / ref.abs().max())


@pytest.mark.parametrize("rfi", [False, True])
@pytest.mark.parametrize("plan", PLANS, ids=lambda p: f"{p[0]}-{p[1]}-{p[2]}")
def test_fused_preop_poly_matches_unfused(C, monkeypatch, plan, rfi):
    spec = _spec(plan[0])
    df = _narrow_df(plan[0])
    ref = _reference(C, spec, df, DM, rfi)
    monkeypatch.setenv("SRTB_DEDISP_POLY", "0")
    (old,), (old_poly,) = _fused(C, spec, plan, df, [DM], rfi)
    monkeypatch.delenv("SRTB_DEDISP_POLY")
    (new,), (new_poly,) = _fused(C, spec, plan, df, [DM], rfi)
    assert not old_poly and new_poly
    e_old, e_new = _max_err(old, ref), _max_err(new, ref)
    print(f"plan {plan} rfi={rfi}: max err poly {e_new:.3e}, "
          f"per-bin fp64 {e_old:.3e} (of max |ref|)")
    # zapped bins are exact zeros on both paths: the zap decisions agree
    assert e_old < 1e-4
    assert e_new <= 2.0 * e_old


@pytest.mark.parametrize("rfi", [False, True])
@pytest.mark.parametrize("plan", SAME_AS_DEFAULT_PLANS,
                         ids=lambda p: f"{p[0]}-{p[1]}-{p[2]}")
def test_fused_preop_poly_matches_per_bin_path(C, monkeypatch, plan, rfi):
    """Same plan, same input, only the phase factors differ.  By Parseval the
    relative L2 difference of the outputs is at most the largest phase
    difference.  Per path that is one f32 rounding of the argument (2.4e-7
    rad below 2 pi for the per-bin path, 9.4e-8 rad below half a turn for the
    polynomial), the per-bin path's f32 scaling by 1/(2 pi) (1.9e-7 rad) and
    1-ulp sine / cosine results (1.2e-7 rad each path): 8e-7 rad together.
    The fp32 FFT behind it turns a 1e-6 input change into no more than that
    again; 2e-6 covers both, and an indexing mistake in the polynomial's
    origin or step is an error of order 1."""
    spec = _spec(plan[0])
    df = _narrow_df(plan[0])
    (new,), (new_poly,) = _fused(C, spec, plan, df, [DM], rfi)
    monkeypatch.setenv("SRTB_DEDISP_POLY", "0")
    (old,), (old_poly,) = _fused(C, spec, plan, df, [DM], rfi)
    assert new_poly and not old_poly
    assert torch.equal(torch.view_as_real(old),
                       torch.view_as_real(_reference(C, spec, df, DM, rfi)))
    rel = float(torch.linalg.vector_norm(new - old) /
                torch.linalg.vector_norm(old))
    print(f"plan {plan} rfi={rfi}: |poly - per-bin| / |per-bin| = {rel:.3e}")
    assert rel <= 2e-6


@pytest.mark.parametrize("plan", PLANS[:1] + SAME_AS_DEFAULT_PLANS[:1],
                         ids=lambda p: f"{p[0]}-{p[1]}-{p[2]}")
def test_wide_columns_fall_back_bit_exact(C, monkeypatch, plan):
    spec = _spec(plan[0])
    df = _wide_df(plan[0])
    (new,), (new_poly,) = _fused(C, spec, plan, df, [DM], True)
    monkeypatch.setenv("SRTB_DEDISP_POLY", "0")
    (old,), (old_poly,) = _fused(C, spec, plan, df, [DM], True)
    assert not new_poly and not old_poly
    assert torch.equal(torch.view_as_real(new), torch.view_as_real(old))
    assert _max_err(new, _reference(C, spec, df, DM, True)) < 1e-4


def test_dm_override_decides_per_call(C, monkeypatch):
    # the bound scales with |dm|: the J1644 value sits ten times under it,
    # a hundred times that DM is over it — on the same plan
    plan = PLANS[0]
    spec = _spec(plan[0])
    df = _narrow_df(plan[0])
    dms = [DM, 100.0 * DM]
    outs, poly = _fused(C, spec, plan, df, dms, False)
    assert list(poly) == [True, False]
    monkeypatch.setenv("SRTB_DEDISP_POLY", "0")
    olds, old_poly = _fused(C, spec, plan, df, dms, False)
    assert list(old_poly) == [False, False]
    refs = [_reference(C, spec, df, dm, False) for dm in dms]
    e_old = _max_err(olds[0], refs[0])
    e_new = _max_err(outs[0], refs[0])
    print(f"dm override: max err poly {e_new:.3e}, per-bin fp64 {e_old:.3e}")
    assert e_new <= 2.0 * e_old
    assert torch.equal(torch.view_as_real(outs[1]),
                       torch.view_as_real(olds[1]))
    assert _max_err(outs[1], refs[1]) < 1e-4
