"""GPU tests of the per-channel normalisation before the incoherent DM-offset
search: the update and apply kernels, the streaming IncoherentSearch with the
feature on and off, and both applications.

Oracle: srtb_amd.ref.incoherent_norm_* and CpuIncoherentSearch.  Where the
input makes every float64 sum exact (small integers, a power-of-two R) the
comparison is bit for bit; the real-valued bounds are derived next to their
asserts.
"""

import os
import subprocess

import numpy as np
import pytest
import torch

from srtb_amd import ref

pytestmark = pytest.mark.gpu

SHAPES = [(2, 1), (64, 96), (67, 37), (130, 1028)]


@pytest.fixture(scope="module")
def C():
    from srtb_amd.ops import native
    torch.cuda.set_device(0)
    return native()


def zero_state(Cn):
    return (torch.zeros(Cn, dtype=torch.float64).cuda(),
            torch.zeros(Cn, dtype=torch.float64).cuda(),
            torch.zeros(Cn, dtype=torch.float32).cuda())


def update(C, plane, alpha, state):
    """One step on the GPU; returns (M, V, G, live) as numpy."""
    M, V, G = state
    live = C.incoh_norm_update(torch.from_numpy(plane).cuda(), alpha, M, V, G)
    return M.cpu().numpy(), V.cpu().numpy(), G.cpu().numpy(), live


def gamma_plane(R, Cn, seed):
    return np.random.default_rng(seed).gamma(16, 1, (R, Cn)).astype(np.float32)


def f32_ulp_close(a, b, ulps=1):
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    return np.abs(a.astype(np.float64) - b.astype(np.float64)) <= \
        ulps * np.spacing(np.maximum(np.abs(a), np.abs(b))).astype(np.float64)


# ---- 1. update kernel ----

@pytest.mark.parametrize("R,Cn", [(2, 1), (64, 96), (64, 37), (128, 1028)])
def test_update_exact_on_small_integers(C, R, Cn):
    """Integers 0..15 and a power-of-two R: every float64 sum, s / R and
    s2 / R is exact, and the update is the same two IEEE operations on both
    sides, so M and V are bit-equal over alpha = 1, 1/2, 1/4."""
    rng = np.random.default_rng(R * 7 + Cn)
    state = zero_state(Cn)
    M = np.zeros(Cn)
    V = np.zeros(Cn)
    for alpha in (1.0, 0.5, 0.25):
        plane = rng.integers(0, 16, (R, Cn)).astype(np.float32)
        m, v = ref.incoherent_norm_stats(plane)
        M = M + np.float64(alpha) * (m - M)
        V = V + np.float64(alpha) * (v - V)
        gM, gV, gG, live = update(C, plane, alpha, state)
        assert np.array_equal(gM, M), np.argwhere(gM != M)[:4]
        assert np.array_equal(gV, V), np.argwhere(gV != V)[:4]
        want_G = ref.incoherent_norm_gain(V)
        assert f32_ulp_close(gG, want_G).all()
        assert np.array_equal(gG > 0, V > 0)
        assert live == int((V > 0).sum())


@pytest.mark.parametrize("R,Cn", SHAPES)
def test_update_real_values_within_the_bounds(C, R, Cn):
    """Gamma noise of shape 16 (mean 16, sigma 4): the first sample lies
    within 6 sigma of the mean (checked).  A sequential float64 sum of R
    terms and the division: m within (R + 1) * 2^-53 relative; the shifted
    sums cancel by at most 1 + 6^2 = 37 < 40: v within 40 * (R + 1) * 2^-53."""
    plane = gamma_plane(R, Cn, 100 + R)
    P64 = plane.astype(np.float64)
    want_m, want_v = P64.mean(axis=0), P64.var(axis=0)
    assert (np.abs(P64[0] - want_m) <= 6 * np.sqrt(want_v)).all()
    gM, gV, gG, live = update(C, plane, 1.0, zero_state(Cn))
    err_m = np.abs(gM - want_m) / np.abs(want_m)
    err_v = np.abs(gV - want_v) / want_v
    print("m err / bound", err_m.max() / ((R + 1) * 2.0 ** -53),
          "v err / bound", err_v.max() / (40 * (R + 1) * 2.0 ** -53))
    assert (err_m <= (R + 1) * 2.0 ** -53).all()
    assert (err_v <= 40 * (R + 1) * 2.0 ** -53).all()
    m, v = ref.incoherent_norm_stats(plane)
    assert f32_ulp_close(gG, ref.incoherent_norm_gain(v)).all()
    assert live == Cn


@pytest.mark.parametrize("R,Cn", [(67, 37), (130, 1028)])
def test_update_dead_channels(C, R, Cn):
    plane = gamma_plane(R, Cn, 200 + R)
    plane[:, 1] = np.float32(1234.5678)
    plane[:, Cn - 2] = 0
    gM, gV, gG, live = update(C, plane, 1.0, zero_state(Cn))
    for c, value in ((1, np.float32(1234.5678)), (Cn - 2, 0.0)):
        assert gV[c] == 0.0 and gG[c] == 0.0 and gM[c] == np.float64(value)
    assert live == Cn - 2 and int((gG > 0).sum()) == Cn - 2


def test_update_is_deterministic(C):
    R, Cn = 130, 1028
    planes = [gamma_plane(R, Cn, 300 + i) for i in range(3)]

    def run():
        state = zero_state(Cn)
        for i, p in enumerate(planes):
            out = update(C, p, 1.0 / (i + 1), state)
        return out

    first = run()
    again = run()
    for a, b in zip(first[:3], again[:3]):
        assert a.tobytes() == b.tobytes()
    assert first[3] == again[3]


def test_update_and_apply_reject_bad_arguments(C):
    f32 = lambda *s: torch.zeros(*s, dtype=torch.float32).cuda()  # noqa: E731
    f64 = lambda *s: torch.zeros(*s, dtype=torch.float64).cuda()  # noqa: E731
    ok = lambda: (f32(8, 4), 1.0, f64(4), f64(4), f32(4))  # noqa: E731
    C.incoh_norm_update(*ok())
    for i, bad, match in [
            (0, f32(8, 4).double(), "float32"), (0, f32(8, 5), "float64"),
            (0, f32(0, 4), "R, C >= 1"), (0, f32(8, 8)[:, ::2], "contiguous"),
            (0, torch.zeros(8, 4), "GPU"), (1, 0.0, "alpha"),
            (1, 1.5, "alpha"), (2, f32(4), "float64"), (3, f64(5), "float64"),
            (4, f64(4), "float32"), (4, f32(8)[::2], "contiguous"),
            (2, torch.zeros(4, dtype=torch.float64), "GPU")]:
        args = list(ok())
        args[i] = bad
        with pytest.raises(RuntimeError, match=match):
            C.incoh_norm_update(*args)

    ok = lambda: (f32(8, 4), f64(4), f32(4), f32(12, 4), 0)  # noqa: E731
    C.incoh_norm_apply(*ok())
    for i, bad, match in [
            (0, f32(8, 4).double(), "float32"), (0, f32(0, 4), "R, C >= 1"),
            (0, f32(8, 8)[:, ::2], "contiguous"), (1, f32(4), "float64"),
            (1, f64(3), "float64"), (2, f64(4), "float32"),
            (3, f32(7, 4), "ring must be"),      # ring_rows < R
            (3, f32(12, 5), "ring must be"), (3, f32(12, 4).double(), "ring"),
            (3, torch.zeros(12, 4), "GPU"),
            (4, 12, "write_row"), (4, -1, "write_row")]:  # >= ring_rows
        args = list(ok())
        args[i] = bad
        with pytest.raises(RuntimeError, match=match):
            C.incoh_norm_apply(*args)


# ---- 2. apply kernel ----

SENTINEL = np.float32(-777.25)


def offset_view(t):
    """The same values in storage that starts one float off 16 bytes."""
    flat = torch.empty(t.numel() + 1, dtype=t.dtype, device=t.device)
    view = flat[1:].view(t.shape)
    view.copy_(t)
    assert view.is_contiguous() and view.data_ptr() % 16 == 4
    return view


@pytest.mark.parametrize("R,Cn", SHAPES)
def test_apply_is_the_float32_map_bit_for_bit(C, R, Cn):
    """From the GPU's own M and G, through the 16-byte path (C = 96, 1028)
    and the scalar path (C = 1, 37, and the two others forced onto it by a
    plane, or a ring, that starts one float off 16 bytes)."""
    plane = gamma_plane(R, Cn, 400 + R)
    plane[:, Cn // 2] *= np.float32(300)
    state = zero_state(Cn)
    gM, gV, gG, _ = update(C, plane, 1.0, state)
    M, _, G = state
    want = ref.incoherent_norm_apply(plane, gM, gG)
    assert want.dtype == np.float32 and np.isfinite(want).all()
    dev = torch.from_numpy(plane).cuda()
    assert dev.data_ptr() % 16 == 0
    geometries = [
        (R, 0),                   # the ring is the block
        (R + 5, R + 2),           # a wrap inside the block
        (2 * R + 7, R + 3),       # D_max > R, no wrap
        (2 * R + 7, 2 * R + 6),   # D_max > R, wrap after one row
    ]
    variants = [(dev, False)]
    if Cn % 4 == 0:
        variants += [(offset_view(dev), False), (dev, True)]
    for ring_rows, write_row in geometries:
        rows = (write_row + np.arange(R)) % ring_rows
        for src, ring_off in variants:
            ring = torch.full((ring_rows, Cn), float(SENTINEL)).cuda()
            if ring_off:
                ring = offset_view(ring)
            C.incoh_norm_apply(src, M, G, ring, write_row)
            got = ring.cpu().numpy()
            assert got[rows].tobytes() == want.tobytes(), \
                (ring_rows, write_row, ring_off,
                 np.argwhere(got[rows] != want)[:4])
            others = np.setdiff1d(np.arange(ring_rows), rows)
            assert (got[others] == SENTINEL).all()


# ---- 3. streaming ----

STREAM = dict(fch1=1500.0, foff=-1.0, tsamp=1e-3,
              offsets=[-100.0, -50.0, 0.0, 50.0, 100.0], snr_threshold=2.0,
              max_boxcar=4)
R_S, C_S, K_S = 64, 96, 4
DEAD = {3: 42.0, 60: 0.0}


def dyadic_planes(n):
    """Planes whose normalised rows are exact: per block and channel a
    permutation of m + s * d, d a fixed multiset of 64 integers with mean 0
    and mean square 4, s a power of two.  Every block has the same statistics
    (mean m, variance 4 s^2, gain 1 / (2 s)), so the running state is exact
    for any alpha and X' = d / 2 in {0, +-0.5, +-1, +-2}: all sums downstream
    are exact in float32 and float64.  Two channels are dead."""
    d = np.array([4, -4] * 5 + [2, -2] * 10 + [1, -1] * 8 + [0] * 18,
                 dtype=np.float64)
    assert d.size == R_S and d.sum() == 0 and (d * d).sum() == 4 * R_S
    rng = np.random.default_rng(21)
    mean = rng.integers(0, 1000, C_S).astype(np.float64)
    scale = 2.0 ** (np.arange(C_S) % 5)
    planes = []
    for _ in range(n):
        p = np.stack([mean[c] + scale[c] * rng.permutation(d)
                      for c in range(C_S)], axis=1)
        for c, value in DEAD.items():
            p[:, c] = value
        planes.append(p.astype(np.float32))
    return planes, mean, scale


def run_stream(gpu, dev_planes):
    """two in flight, as the engine's two slots"""
    out, pending = [], []
    for p in dev_planes:
        pending.append(gpu.submit_plane(p))
        if len(pending) == 2:
            k = pending.pop(0)
            out.append((gpu.wait(k), gpu.plane(k).numpy()))
    for k in pending:
        out.append((gpu.wait(k), gpu.plane(k).numpy()))
    return out


def test_streaming_matches_the_cpu_search(C):
    from tests.test_gpu_incoherent import same_result
    gpu = C.IncoherentSearch(rows=R_S, channels=C_S, normalize=True,
                             normalize_blocks=K_S, **STREAM)
    cpu = ref.CpuIncoherentSearch(R_S, C_S, normalize=True,
                                  normalize_blocks=K_S, **STREAM)
    assert gpu.d_max == cpu.d_max == 26
    planes, mean, scale = dyadic_planes(8)
    dev = [torch.from_numpy(p).cuda() for p in planes]
    live = C_S - len(DEAD)
    counts = []

    def compare(dev_part, planes_part, first_block):
        for b, ((res, Y), p) in enumerate(zip(run_stream(gpu, dev_part),
                                              planes_part), first_block):
            want = cpu.add(p)
            same_result(res, want)  # valid, first_row, block, detections
            assert res["block"] == b
            assert res["live_channels"] == want["live_channels"] == live
            assert np.array_equal(Y, want["Y"].astype(np.float32))
            assert res["valid"] == (b >= 1)
            counts.extend(ln["count"] for tr in res["trials"]
                          for ln in tr["lengths"])
        assert np.array_equal(gpu.norm_mean().numpy(), cpu.M)
        assert np.array_equal(gpu.norm_var().numpy(), cpu.V)
        assert np.array_equal(gpu.norm_gain().numpy(), cpu.G)

    compare(dev[:5], planes[:5], 0)
    alive = np.array([c not in DEAD for c in range(C_S)])
    assert np.array_equal(cpu.M[alive], mean[alive])
    assert np.array_equal(cpu.V[alive], (4 * scale * scale)[alive])
    assert counts and max(counts) > 0  # the detections compared are not empty

    gpu.reset()
    cpu.reset()
    assert not gpu.norm_mean().numpy().any()
    assert not gpu.norm_var().numpy().any()
    assert not gpu.norm_gain().numpy().any()
    compare(dev[5:], planes[5:], 0)


def drifting_planes():
    """The loud-channel planes with a level that rises by a tenth per block,
    so the running state depends on alpha in every block."""
    from tests.test_incoherent_norm_cpu import loud_channel_planes
    return [(p * np.float32(1 + 0.1 * b)).astype(np.float32)
            for b, p in enumerate(loud_channel_planes())]


def test_streaming_state_follows_alpha_into_the_exponential_regime(C):
    """K = 4 over 8 drifting blocks, a reset after block 4: the clamp of
    alpha = 1 / min(b + 1, K) acts from the fifth block of the first run on.
    The state is compared with the oracle's after every block, one block in
    flight.

    Bounds.  M and V are convex combinations of block statistics, each
    within (R + 1) * 2^-53 (m) and 40 * (R + 1) * 2^-53 (v) relative of the
    true one, plus three roundings per block and update; two such results
    differ by at most twice that.  The float32 roundings of two such M are
    equal or adjacent, G agrees to 1 ulp, and the subtraction and the
    multiplication round once each on both sides, so a normalised sample
    differs by at most e = spacing32(M) * G * (1 + 2^-22) + 2^-22 * |X'|.
    Y sums C of them in float32: |Y - Y64| <= sum of e over the gathered
    samples + C * 2^-24 * sum |X'|, the bound of test_gpu_incoherent.  The
    rows of Y have an rms near sqrt(C) ~ 10 and differ by less than 1e-3,
    so snr = peak / rms agrees to 1e-3 absolute with a wide margin."""
    kw = dict(STREAM, snr_threshold=3.0)
    gpu = C.IncoherentSearch(rows=R_S, channels=C_S, normalize=True,
                             normalize_blocks=K_S, **kw)
    cpu = ref.CpuIncoherentSearch(R_S, C_S, normalize=True,
                                  normalize_blocks=K_S, **kw)
    # what a searcher that ignored K, or never clamped, would hold
    wrong = [ref.CpuIncoherentSearch(R_S, C_S, normalize=True,
                                     normalize_blocks=k, **kw)
             for k in (8, 65536, 1)]
    planes = drifting_planes()
    dev = [torch.from_numpy(p).cuda() for p in planes]
    u = 2.0 ** -53

    def compare(dev_part, planes_part):
        stats = []
        e_chan = np.zeros(C_S)
        for b, (d, p) in enumerate(zip(dev_part, planes_part)):
            k = gpu.submit_plane(d)
            res, Y = gpu.wait(k), gpu.plane(k).numpy()
            want = cpu.add(p)
            others = [w.add(p) for w in wrong]
            for key in ("valid", "first_row", "block", "live_channels"):
                assert res[key] == want[key], (b, key)
            assert res["block"] == b and res["live_channels"] == C_S
            assert res["valid"] == (b >= 1)

            stats.append(ref.incoherent_norm_stats(p))
            m_max = np.max([np.abs(m) for m, _ in stats], axis=0)
            v_max = np.max([v for _, v in stats], axis=0)
            tol_m = 2 * (R_S + 1 + 3 * (b + 1)) * u * m_max
            tol_v = 2 * (40 * (R_S + 1) + 3 * (b + 1)) * u * v_max
            gM, gV = gpu.norm_mean().numpy(), gpu.norm_var().numpy()
            gG = gpu.norm_gain().numpy()
            assert (np.abs(gM - cpu.M) <= tol_m).all(), b
            assert (np.abs(gV - cpu.V) <= tol_v).all(), b
            assert f32_ulp_close(gG, cpu.G).all(), b
            # the comparison tells the right alpha from the wrong ones
            for w, acts in zip(wrong, (b >= K_S, b >= K_S, b >= 1)):
                if acts:
                    assert (np.abs(w.M - cpu.M) > 1e6 * tol_m).all(), b
                    assert (np.abs(gM - w.M) > 1e6 * tol_m).all(), b

            # rows of earlier blocks were normalised by earlier states: the
            # largest spacing32(M) * G so far; rows from before the stream
            # are zero on both sides
            step = np.spacing(np.abs(cpu.M).astype(np.float32)).astype(
                np.float64) * cpu.G * (1 + 2.0 ** -22)
            e_chan[:] = np.maximum(e_chan, step)
            x = np.abs(cpu.window)
            e = np.tile(e_chan, (len(x), 1))
            e[~x.any(axis=1)] = 0
            e += 2.0 ** -22 * x
            bound = ref.incoherent_dedisperse(e, cpu.delays, R_S) + \
                C_S * 2.0 ** -24 * ref.incoherent_dedisperse(
                    x, cpu.delays, R_S)
            err = np.abs(Y.astype(np.float64) - want["Y"])
            some = bound > 0
            print("block", b, "max Y err / bound",
                  (err[some] / bound[some]).max(), "max Y err", err.max())
            assert (err <= bound).all(), b
            assert err.max() < 1e-3
            for g, w in zip(res["trials"], want["trials"]):
                for gl, wl in zip(g["lengths"], w["lengths"]):
                    assert abs(gl["snr"] - wl["snr"]) <= 1e-3, (b, gl, wl)
                    assert gl["boxcar_length"] == wl["boxcar_length"]

    compare(dev[:5], planes[:5])
    gpu.reset()
    cpu.reset()
    for w in wrong:
        w.reset()
    assert not gpu.norm_mean().numpy().any()
    compare(dev[5:], planes[5:])


def test_normalize_off_is_bit_identical_to_the_search_without_it(C):
    from tests.test_incoherent_norm_cpu import loud_channel_planes
    kw = dict(STREAM, snr_threshold=3.0)
    plain = C.IncoherentSearch(rows=R_S, channels=C_S, **kw)
    off = C.IncoherentSearch(rows=R_S, channels=C_S, normalize=False,
                             normalize_blocks=3, **kw)
    dev = [torch.from_numpy(p).cuda() for p in loud_channel_planes()]
    seen = 0
    for (r0, y0), (r1, y1) in zip(run_stream(plain, dev),
                                  run_stream(off, dev)):
        assert y0.tobytes() == y1.tobytes()
        assert r0 == r1
        assert r0["live_channels"] == 0
        seen += r0["valid"]
    assert seen == 7
    with pytest.raises(RuntimeError, match="without normalize"):
        off.norm_mean()


@pytest.mark.parametrize("K", [0, 65537, -1])
def test_constructor_rejects_k_out_of_range(C, K):
    for normalize in (True, False):
        with pytest.raises(RuntimeError, match="normalize_blocks"):
            C.IncoherentSearch(rows=R_S, channels=C_S, normalize=normalize,
                               normalize_blocks=K, **STREAM)


# ---- 4. the loud-channel case: fails without the feature ----

def test_loud_channels_submit_plane_against_the_oracle(C):
    """CPU oracle on this input: with the feature on exactly one candidate
    (block 5, offset 50, length 1, row 330, snr 7.61; every other (trial,
    length) below 5.38); off: none, best snr 3.93."""
    from tests.test_incoherent_norm_cpu import (
        LOUD, LOUD_CANDIDATE, all_detections, candidates_of, cpu_search,
        loud_channel_planes)
    planes = loud_channel_planes()
    dev = [torch.from_numpy(p).cuda() for p in planes]
    kw = dict(LOUD)
    R, Cn = kw.pop("R"), kw.pop("C")

    gpu_off = C.IncoherentSearch(rows=R, channels=Cn, **kw)
    off = [res for res, _ in run_stream(gpu_off, dev)]
    assert candidates_of(off) == []

    gpu = C.IncoherentSearch(rows=R, channels=Cn, normalize=True, **kw)
    cpu = cpu_search(normalize=True)
    on = [res for res, _ in run_stream(gpu, dev)]
    want = [cpu.add(p) for p in planes]
    for res, w in zip(on, want):
        for key in ("valid", "first_row", "block", "live_channels"):
            assert res[key] == w[key]
    cands, want_cands = candidates_of(on), candidates_of(want)
    print("gpu", cands, "cpu", want_cands)
    assert len(cands) == len(want_cands) == 1
    assert cands[0][2:] == want_cands[0][2:] == LOUD_CANDIDATE
    assert cands[0][1] == 1
    assert abs(cands[0][0] - want_cands[0][0]) <= 1e-3 * want_cands[0][0]
    assert max(d[0] for d in all_detections(on)
               if d[2:] != cands[0][2:]) < 5.5

    # The state against the oracle's.  Both are convex combinations of block
    # statistics, each within (R + 1) * 2^-53 (m) and 40 * (R + 1) * 2^-53
    # (v) relative of the true one, plus three roundings per block and
    # update; two such results differ by at most twice that.
    B = len(planes)
    stats = [ref.incoherent_norm_stats(p) for p in planes]
    m_max = np.max([np.abs(m) for m, _ in stats], axis=0)
    v_max = np.max([v for _, v in stats], axis=0)
    gM, gV = gpu.norm_mean().numpy(), gpu.norm_var().numpy()
    assert (np.abs(gM - cpu.M) <= 2 * (R + 1 + 3 * B) * 2.0 ** -53
            * m_max).all()
    assert (np.abs(gV - cpu.V) <= 2 * (40 * (R + 1) + 3 * B) * 2.0 ** -53
            * v_max).all()
    assert f32_ulp_close(gpu.norm_gain().numpy(), cpu.G).all()


# ---- 5. applications ----

OFFSETS = "-2,-1,0,1,2,3,4"


def backend_binary():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    binary = os.path.join(root, "bin", "srtb-backend")
    assert os.path.exists(binary), "native binaries not built"
    return binary


def test_both_apps_write_the_same_normalised_candidates(tmp_path):
    from srtb_amd.main import main
    from tests.test_incoherent_cpu import (APP_ARGS, check_candidates,
                                           offset_pulse_recording)
    binary = backend_binary()
    rec = tmp_path / "rec.bin"
    offset_pulse_recording(rec)
    args = APP_ARGS + ["--input_file_path", str(rec),
                       "--incoherent_dm_offsets", OFFSETS]
    files = {}
    # the key on with K = 4, off, and on with K = 1: the recording has three
    # blocks, so K = 1 (alpha = 1 throughout) differs from K = 4 from the
    # second block on, and an app that dropped the key would show
    for key, K in (("1", "4"), ("0", "4"), ("1", "1")):
        py_out = tmp_path / f"py{key}{K}.cand"
        cc_out = tmp_path / f"cc{key}{K}.cand"
        keys = ["--incoherent_normalize", key,
                "--incoherent_normalize_blocks", K]
        assert main(args + keys + [
            "--device", "cuda", "--incoherent_output_path", str(py_out),
            "--baseband_output_file_prefix", f"{tmp_path}/p{key}{K}_"]) == 0
        run = subprocess.run(
            ["timeout", "-k", "10", "120", binary] + args + keys +
            ["--incoherent_output_path", str(cc_out),
             "--baseband_output_file_prefix", f"{tmp_path}/c{key}{K}_"],
            capture_output=True, text=True, timeout=150)
        assert run.returncode == 0, run.stderr
        check_candidates(py_out)
        assert cc_out.read_bytes() == py_out.read_bytes()
        files[key, K] = py_out.read_bytes()
    assert files["1", "4"] != files["0", "4"]
    assert files["1", "1"] != files["1", "4"]
    assert files["1", "1"] != files["0", "4"]


def test_both_apps_reject_the_bad_key_combinations(tmp_path):
    from srtb_amd.main import main
    from tests.test_incoherent_cpu import APP_ARGS
    binary = backend_binary()
    base = APP_ARGS + ["--input_file_path", "none.bin"]
    search = ["--incoherent_dm_offsets", "0,1",
              "--incoherent_output_path", "c.cand"]
    for extra, word in [
            (["--incoherent_normalize", "1"],
             "incoherent_normalize needs incoherent_dm_offsets"),
            (search + ["--incoherent_normalize", "1",
                       "--incoherent_normalize_blocks", "0"],
             "incoherent_normalize_blocks must be 1 .. 65536"),
            (search + ["--incoherent_normalize", "1",
                       "--incoherent_normalize_blocks", "65537"],
             "incoherent_normalize_blocks must be 1 .. 65536"),
            (search + ["--incoherent_normalize", "1",
                       "--incoherent_normalize_blocks", "-3"],
             "incoherent_normalize_blocks must be 1 .. 65536"),
            # the range holds with the feature off, as in the constructor
            (["--incoherent_normalize_blocks", "0"],
             "incoherent_normalize_blocks must be 1 .. 65536")]:
        run = subprocess.run([binary] + base + extra, capture_output=True,
                             text=True, timeout=60, cwd=tmp_path)
        assert run.returncode == 2, (extra, run.stdout, run.stderr)
        assert word in run.stdout + run.stderr
        with pytest.raises(SystemExit, match=word):
            main(base + ["--device", "cuda"] + extra)
