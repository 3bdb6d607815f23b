"""GPU tests of the full-Stokes filterbank output: the polarization-product
kernel, the PolCombiner that joins two engines without a host sync, and both
apps writing one nifs = 4 file from a two-polarization recording.

Oracle: srtb_amd.ref.pol_products_block in float64, fed with small-integer
waterfalls whose sums are exact in float32 (stand-alone kernel, compared
bitwise) or with the GPU's own unzapped waterfalls and flags (engine tests).
"""

import glob
import os
import subprocess

import numpy as np
import pytest
import torch

from srtb_amd import ref
from srtb_amd.config import Config
from srtb_amd.io.writers import filterbank_header, read_filterbank
from srtb_amd.pipeline.cpu import synthesize_dispersed_pulse
from tests.test_gpu_filterbank import (KERNEL_CASES, TONE_ROW, N, S, L,
                                       check_quantised, make_block,
                                       make_engine, pattern_waterfall)

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "bin", "srtb-backend")

STATES = ("I", "AABBCRCI", "IQUV")


@pytest.fixture(scope="module")
def C():
    from srtb_amd.ops import native
    torch.cuda.set_device(0)
    return native()


def pattern_b(S_, L_):
    """A second small-integer pattern, |.|^2 <= 202, with other multipliers
    than pattern_waterfall: swapping A and B or a wrong conjugate sign changes
    the products."""
    t = np.arange(L_)[None, :]
    r = np.arange(S_)[:, None]
    re = (t * 3 + r * 13) % 23 - 11
    im = (t * 11 + r * 5) % 19 - 9
    return (re + 1j * im).astype(np.complex64)


def flag_cases(S_):
    """none, A only, B only, both on different rows."""
    def flags(rows):
        f = np.zeros(S_, dtype=np.uint8)
        f[list(rows)] = 1
        return f
    return [(None, None), (flags({0, S_ // 2}), None),
            (None, flags({S_ - 1})), (flags({0}), flags({S_ - 1}))]


def dev(a):
    return None if a is None else torch.from_numpy(a).cuda()


SHAPES = [case[1:] for case in KERNEL_CASES]


# ---- 1. kernel, bit-exact on small integers ----

@pytest.mark.parametrize("reverse", [False, True])
@pytest.mark.parametrize("S_,L_,V,tscrunch,fscrunch", SHAPES)
def test_pol_kernel_exact(C, S_, L_, V, tscrunch, fscrunch, reverse):
    a, b = pattern_waterfall(S_, L_), pattern_b(S_, L_)
    da, db = dev(a), dev(b)
    for fa, fb in flag_cases(S_):
        dfa, dfb = dev(fa), dev(fb)
        for state in STATES:
            want = ref.pol_products_block(a, b, V, tscrunch, fscrunch, reverse,
                                          state, flags_a=fa, flags_b=fb)
            # every partial sum is an integer below 2^24: exact in float32
            assert np.abs(want).max() < 2 ** 24
            got = C.filterbank_detect_pol(
                da, db, dfa, dfb, V, tscrunch, fscrunch, reverse,
                ref.POL_STATES[state]).cpu().numpy()
            assert got.dtype == np.float32
            assert got.shape == (V // tscrunch, ref.POL_STATE_NIFS[state],
                                 S_ // fscrunch)
            want32 = want.astype(np.float32)
            assert np.array_equal(got, want32), (
                state, fa is not None, fb is not None,
                np.argwhere(got != want32)[:8])


# ---- 2. the I plane is the sum of the two per-stream planes ----

@pytest.mark.parametrize("reverse", [False, True])
@pytest.mark.parametrize("S_,L_,V,tscrunch,fscrunch", SHAPES)
def test_intensity_is_the_sum_of_both_detects(C, S_, L_, V, tscrunch, fscrunch,
                                              reverse):
    da, db = dev(pattern_waterfall(S_, L_)), dev(pattern_b(S_, L_))
    got = C.filterbank_detect_pol(da, db, None, None, V, tscrunch, fscrunch,
                                  reverse, ref.POL_STATES["I"])
    want = (C.filterbank_detect(da, None, V, tscrunch, fscrunch, reverse)
            + C.filterbank_detect(db, None, V, tscrunch, fscrunch, reverse))
    assert torch.equal(got[:, 0, :], want)


# ---- 3. identities ----

def test_pol_kernel_identities(C):
    S_, L_, V, t, f = 66, 200, 200, 4, 2
    a = pattern_waterfall(S_, L_)

    def iquv(b):
        p = C.filterbank_detect_pol(dev(a), dev(b.astype(np.complex64)), None,
                                    None, V, t, f, False,
                                    ref.POL_STATES["IQUV"]).cpu().numpy()
        return (p[:, k] for k in range(4))

    i, q, u, v = iquv(a)
    assert (i > 0).all()
    assert (q == 0).all() and np.array_equal(u, i) and (v == 0).all()
    i, q, u, v = iquv(1j * a)
    assert np.array_equal(v, -i) and (u == 0).all() and (q == 0).all()
    i, q, u, v = iquv(-1j * a)
    assert np.array_equal(v, i) and (u == 0).all()
    i, q, u, v = iquv(0 * a)
    assert np.array_equal(q, i) and (u == 0).all() and (v == 0).all()


# ---- 4. rejections ----

def test_pol_kernel_rejections(C):
    def z(S_, L_):
        return torch.zeros(S_, L_, dtype=torch.complex64).cuda()

    a = z(6, 10)
    for wa, wb, args in [
            (a, z(6, 12), (6, 1, 1, False, 2)),      # mismatched shapes
            (a, z(5, 10), (6, 1, 1, False, 2)),
            (z(6, 9), z(6, 9), (6, 1, 1, False, 2)),  # odd L
            (a, a, (6, 3, 1, False, 2)),             # tscrunch 3
            (z(2, 8192), z(2, 8192), (8192, 8192, 1, False, 2)),
            (a, a, (6, 1, 4, False, 2)),             # fscrunch does not divide
            (a, a, (11, 1, 1, False, 2)),            # V > L
            (a, a, (6, 1, 1, False, 3)),             # no such state
            (a, a, (6, 1, 1, False, -1))]:
        with pytest.raises(RuntimeError):
            C.filterbank_detect_pol(wa, wb, None, None, *args)
    with pytest.raises(RuntimeError):  # flags of the wrong length
        C.filterbank_detect_pol(a, a, torch.zeros(5, dtype=torch.uint8).cuda(),
                                None, 6, 1, 1, False, 2)


# ---- 5. two engines + combiner against the oracle ----

@pytest.fixture(scope="module")
def raw_a():
    return make_block()


@pytest.fixture(scope="module")
def raw_b():
    """Independent noise, the same dispersed pulse as make_block, no tone."""
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
        rng=np.random.default_rng(1), width=1)
    return torch.from_numpy(raw.copy())


def make_combiner(C, **kw):
    args = dict(n=N, channels=S, nsamps_reserved=0, tscrunch=16, fscrunch=1,
                reverse=True, pol_state=ref.POL_STATES["IQUV"], nbits=32)
    args.update(kw)
    return C.PolCombiner(**args)


def run_pair(ea, eb, comb, raw_a, raw_b):
    """Both engines and the combiner back to back, no host wait in between."""
    sa, sb = ea.submit(raw_a), eb.submit(raw_b)
    k = comb.submit(ea, sa, eb, sb)
    comb.wait(k)
    return sa, sb, k, ea.wait(sa), eb.wait(sb)


@pytest.mark.parametrize("state", ["IQUV", "AABBCRCI"])
@pytest.mark.parametrize("odd_rows", [False, True])
@pytest.mark.parametrize("bandwidth", [64.0, -64.0])
@pytest.mark.parametrize("tscrunch,fscrunch", [(1, 1), (16, 1), (64, 64)])
def test_combiner_matches_oracle(C, raw_a, raw_b, tscrunch, fscrunch,
                                 bandwidth, odd_rows, state):
    reserved = 2 * S * tscrunch * 3 if odd_rows else 0
    ea, eb = (make_engine(C, bandwidth=bandwidth, nsamps_reserved=reserved)
              for _ in range(2))
    comb = make_combiner(C, nsamps_reserved=reserved, tscrunch=tscrunch,
                         fscrunch=fscrunch, reverse=bandwidth > 0,
                         pol_state=ref.POL_STATES[state])
    valid = (N - reserved) // (2 * S)
    R, Cn = valid // tscrunch, S // fscrunch
    assert (comb.rows, comb.nifs, comb.channels) == (R, 4, Cn)
    if odd_rows:
        assert R % 2 == 1 and valid != ea.ts_count
    sa, sb, k, _, _ = run_pair(ea, eb, comb, raw_a, raw_b)
    fa, fb = ea.sk_flags(sa).cpu().numpy(), eb.sk_flags(sb).cpu().numpy()
    assert fa[TONE_ROW] == 1 and fb[TONE_ROW] == 0  # precondition
    wa = ea.waterfall(sa, zap=False).cpu().numpy()
    wb = eb.waterfall(sb, zap=False).cpu().numpy()
    want = ref.pol_products_block(wa, wb, valid, tscrunch, fscrunch,
                                  bandwidth > 0, state, flags_a=fa,
                                  flags_b=fb)
    host = comb.plane(k)
    got = comb.power(k).cpu().numpy()
    assert host.dtype == torch.float32 and tuple(host.shape) == (R, 4, Cn)
    assert np.array_equal(host.numpy(), got)  # pinned mirror = device plane
    i_want = want[:, 0] + want[:, 1] if state == "AABBCRCI" else want[:, 0]
    # three roundings per term, n - 1 for the sum, one for the combination:
    # (n + 3) * 2^-24 * sum|terms|, sum|terms| <= I (Cauchy-Schwarz), times 2
    bound = ((tscrunch * fscrunch + 3) * 2.0 ** -23 * i_want)[:, None, :]
    err = np.abs(got - want)
    print("max err / bound", (err / np.where(bound > 0, bound, 1.0)).max())
    assert (err <= bound).all()
    assert (i_want > 0).any()
    if fscrunch == 1:
        c = S - 1 - TONE_ROW if bandwidth > 0 else TONE_ROW
        assert (got[:, :, c] == 0).all()
    u = got[:, 2].astype(np.float64).sum(axis=1)
    if bandwidth > 0:
        # the dedispersed pulse: the brightest row of I and its neighbours
        i_got = (got[:, 0] + got[:, 1] if state == "AABBCRCI"
                 else got[:, 0]).astype(np.float64).sum(axis=1)
        row = int(np.argmax(i_got))
        assert abs(row - int(0.3 * L) // tscrunch) <= 1
        assert u[max(row - 1, 0):row + 2].sum() > 0
    else:
        # dedispersed with the band mirrored the pulse stays smeared over the
        # block, but it is still common to both polarizations
        assert u.sum() > 0


# ---- 6. event chaining ----

def test_event_chaining_three_blocks(C, raw_a, raw_b):
    ea, eb = make_engine(C), make_engine(C)
    comb = make_combiner(C)
    planes = []
    for want_k in (0, 1, 0):
        sa, sb, k, _, _ = run_pair(ea, eb, comb, raw_a, raw_b)
        assert k == want_k
        plane = comb.plane(k)
        # the stand-alone kernel on the synchronized waterfalls and flags
        again = C.filterbank_detect_pol(
            ea.waterfall(sa, zap=False), eb.waterfall(sb, zap=False),
            ea.sk_flags(sa), eb.sk_flags(sb), L, 16, 1, True,
            ref.POL_STATES["IQUV"]).cpu()
        assert torch.equal(plane, again)
        assert torch.equal(plane, comb.power(k).cpu())
        planes.append(plane)
    assert (planes[0] != 0).any()
    assert torch.equal(planes[0], planes[1])
    assert torch.equal(planes[0], planes[2])


# ---- 7. 8-bit ----

def test_combiner_8bit(C, raw_a, raw_b):
    ea, eb = make_engine(C), make_engine(C)
    comb = make_combiner(C, tscrunch=2, nbits=8)
    _, _, k, _, _ = run_pair(ea, eb, comb, raw_a, raw_b)
    R, P, Cn = comb.rows, comb.nifs, comb.channels
    q = comb.plane(k)
    assert q.dtype == torch.uint8 and tuple(q.shape) == (R, P, Cn)
    power = comb.power(k)
    mean, std = comb.stats(k)
    assert mean.shape == std.shape == (P * Cn,)
    m2, s2 = C.filterbank_channel_stats(power.view(R, P * Cn))
    assert torch.equal(m2.cpu(), mean) and torch.equal(s2.cpu(), std)
    check_quantised(q.numpy().reshape(R, P * Cn),
                    power.cpu().numpy().reshape(R, P * Cn), mean.numpy(),
                    std.numpy())
    c = S - 1 - TONE_ROW
    assert (q.numpy()[:, :, c] == 64).all()
    assert (std.numpy().reshape(P, Cn)[:, c] == 0).all()
    # signed products sit at level 64 as well
    live = np.delete(q.numpy().astype(np.float64), c, axis=2)
    assert np.abs(live.mean(axis=0) - 64).max() < 1.0
    with pytest.raises(RuntimeError, match="8 bits"):
        make_combiner(C).stats(0)


# ---- 8. isolation ----

def test_combiner_leaves_the_engines_unchanged(C, raw_a, raw_b):
    plain = [make_engine(C), make_engine(C)]
    joined = [make_engine(C), make_engine(C)]
    comb = make_combiner(C)
    slots = [e.submit(r) for e, r in zip(plain, (raw_a, raw_b))]
    res = [e.wait(s) for e, s in zip(plain, slots)]
    sa, sb, k, ra, rb = run_pair(joined[0], joined[1], comb, raw_a, raw_b)
    assert [ra, rb] == res
    for e0, s0, e1, s1 in zip(plain, slots, joined, (sa, sb)):
        assert e1.filterbank_rows == 0 and e1.filterbank_channels == 0
        assert torch.equal(e0.time_series(s0), e1.time_series(s1))
        assert torch.equal(torch.view_as_real(e0.waterfall(s0)),
                           torch.view_as_real(e1.waterfall(s1)))
    assert (comb.plane(k) != 0).any()


# ---- 9. constructor and submit rejections ----

@pytest.mark.parametrize("kw,match", [
    (dict(tscrunch=12), "tscrunch"),
    (dict(tscrunch=8192), "tscrunch"),
    (dict(fscrunch=3), "fscrunch"),
    (dict(nbits=16), "nbits"),
    (dict(tscrunch=16, nsamps_reserved=2 * S * 8), "nsamps_reserved"),
    (dict(pol_state=3), "pol_state"),
])
def test_combiner_constructor_rejections(C, kw, match):
    with pytest.raises(RuntimeError, match=match):
        make_combiner(C, **kw)


def test_combiner_rejects_engines_of_another_shape(C, raw_a):
    ea, eb = make_engine(C), make_engine(C, channels=S // 2)
    comb = make_combiner(C)
    sa, sb = ea.submit(raw_a), eb.submit(raw_a)
    with pytest.raises(RuntimeError, match="spectrum_channel_count"):
        comb.submit(ea, sa, eb, sb)
    ea.wait(sa)
    eb.wait(sb)
    with pytest.raises(RuntimeError, match="spectrum_channel_count"):
        make_combiner(C, channels=S // 2).submit(ea, sa, ea, sa)


# ---- 10. srtb_amd.main, GPU against CPU ----

@pytest.fixture(scope="module")
def two_pol_files(tmp_path_factory):
    """The two-pol recording through srtb_amd.main on the GPU and on the CPU,
    IQUV at 32 bits."""
    from srtb_amd.main import main
    from tests.test_filterbank_cpu import TWO_POL_ARGS
    from tests.test_main_app import make_2pol_recording
    tmp = tmp_path_factory.mktemp("stokes")
    _, rec = make_2pol_recording(tmp)
    files = {}
    for device in ("cuda", "cpu"):
        (tmp / device).mkdir()
        out = tmp / device / "pol.fil"
        rc = main(TWO_POL_ARGS + [
            "--device", device, "--input_file_path", rec,
            "--filterbank_output_path", str(out),
            "--filterbank_polarization", "IQUV", "--filterbank_nbits", "32",
            "--baseband_output_file_prefix", f"{tmp}/{device}/p2_"])
        assert rc == 0
        files[device] = out
    return tmp, rec, files


def close_to(plane, want):
    """fp32 transforms: errors ~1e-5 of the mean power per cell; 1e-3 of the
    mean is the margin the per-stream GPU-against-CPU file test takes."""
    np.testing.assert_allclose(plane, want, rtol=1e-3,
                               atol=1e-3 * float(want[:, 0].mean()))


def test_main_gpu_file_matches_the_cpu_file(two_pol_files):
    from tests.test_stokes_cpu import check_stokes_file
    tmp, _, files = two_pol_files
    for device in ("cuda", "cpu"):
        check_stokes_file(tmp / device)
    hg, gpu = read_filterbank(str(files["cuda"]))
    hc, cpu = read_filterbank(str(files["cpu"]))
    assert hg == hc and hg["nifs"] == 4
    close_to(gpu, cpu)


# ---- 11. srtb-backend ----

@pytest.mark.skipif(not os.path.exists(BIN), reason="native binaries not built")
def test_srtb_backend_writes_the_same_file(two_pol_files):
    from tests.test_filterbank_cpu import TWO_POL_ARGS
    tmp, rec, files = two_pol_files
    (tmp / "native").mkdir()
    fil = tmp / "native" / "pol.fil"
    out = subprocess.run(
        ["timeout", "-k", "10", "240", BIN, *TWO_POL_ARGS,
         "--input_file_path", rec, "--filterbank_output_path", str(fil),
         "--filterbank_polarization", "IQUV", "--filterbank_nbits", "32",
         "--baseband_output_file_prefix", f"{tmp}/native/out_"],
        capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr
    assert "blocks=2" in out.stdout, (out.stdout, out.stderr)
    assert glob.glob(str(tmp / "native" / "*.fil")) == [str(fil)]

    n, s, t = 1 << 16, 64, 4
    kw = ref.filterbank_header_fields(1400.0, 64.0, 128e6, s, t, 1)
    kw.update(nbits=32, tstart=0.0, nifs=4)
    header = filterbank_header(**kw)
    blob = fil.read_bytes()
    assert blob[:len(header)] == header
    R = n // (2 * s * t)
    assert len(blob) == len(header) + 2 * R * 4 * s * 4
    h, data = read_filterbank(str(fil))
    assert h["nifs"] == 4 and data.shape == (2 * R, 4, s)
    _, gpu = read_filterbank(str(files["cuda"]))
    close_to(data, gpu)
