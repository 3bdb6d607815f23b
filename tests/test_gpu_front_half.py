"""The front half of the chain per sample: unpack, window table and the
forward FFT that decodes raw bytes in its first pass's loads.

A. Every unpack kernel against srtb_amd.ref, bit for bit: the fields are small
   integers and float(field) * w[i] is one correctly rounded float32 product,
   so numpy reproduces the kernel exactly when the window is made on the host
   and passed in.  Shapes: the small ones, and one per kernel past the cap of
   T = 2^20 threads per launch, where the grid-stride loops (unrolled 2 and 4,
   with wave shuffles inside for the sub-byte kernel) make a second and third
   trip.
B. Counts a launcher cannot cover raise instead of leaving a tail of the
   output unwritten; the 8-bit cast covers any count.
C. build_window against float64.
D. native_rfft_raw (decode at load) against native_rfft(unpack(raw)) bit for
   bit, and against float64 in the measure and with the limit of
   test_gpu_fft_accuracy.py, for the seven formats in every first-pass kernel.
E. The same through the mono N = 32 column kernel (SRTB_FFT_PAIR32=0, read
   once per process, hence a child process).
F. submit_samples with a window: the caller applies it, the engine de-applies
   the waterfall window.

Measured on an MI355X: D and E are bit-identical in all 49 instantiations
(they were not for the unsigned formats before dec_opaque() in fft.hip) and at
most 0.59 of the float64 limit; the table is in docs/fft_design.md
("Decode at load against unpack + transform").
"""

import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if __name__ == "__main__":
    sys.path.insert(0, ROOT)

from srtb_amd import ref  # noqa: E402

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
T = 1 << 20  # kMaxBlocks * kBlock: the most threads one launch gets
WRAP = 2 * T + 37  # elements per thread-strided kernel past the cap

FORMATS = [1, 2, 4, 8, -8, 16, -16, 32, -32]
DECODE_FORMATS = [1, 2, 4, 8, -8, 16, -16]

PLANT16 = np.array([0x0000, 0x7fff, 0x8000, 0xffff], dtype="<u2")
PLANT32 = np.array([0x00ffffff, 0x01000001, 0x7fffffff, 0x80000000,
                    0xffffffff], dtype="<u4")


@pytest.fixture(scope="module")
def C():
    from srtb_amd.ops import native
    torch.cuda.set_device(0)
    return native()


def to_gpu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def random_bytes(nbytes, seed, plant=None):
    """Uniform bytes over 0..255; `plant` (little-endian words) overwrites the
    first bytes when it fits."""
    raw = np.random.default_rng(seed).integers(0, 256, nbytes, dtype=np.uint8)
    if plant is not None and plant.nbytes <= nbytes:
        raw[:plant.nbytes] = plant.view(np.uint8)
    return raw


def plant_for(nbits):
    return {16: PLANT16, 32: PLANT32}.get(abs(nbits))


@functools.lru_cache(maxsize=2)
def hamming(n):
    return ref.window_coefficients("hamming", n)


def assert_same(out_t, expect, what):
    """Exact comparison on the device (the 1-bit wrap case is 270 MB); on a
    mismatch report where."""
    exp_t = to_gpu(expect)
    assert out_t.shape == exp_t.shape and out_t.dtype == exp_t.dtype, what
    if torch.equal(out_t, exp_t):
        return
    bad = torch.nonzero(out_t != exp_t).flatten()
    i = int(bad[0])
    raise AssertionError(
        f"{what}: {bad.numel()} of {exp_t.numel()} samples differ, first at "
        f"{i}: got {float(out_t[i])!r}, expected {float(exp_t[i])!r}")


# ---------------- A. unpack, exact ----------------

def raw_bytes_for(nbits, shape):
    """Raw byte count of a named shape."""
    ab = abs(nbits)
    if shape == "small":
        return 1 << 12
    if shape == "wrap":
        if ab < 8:
            # waves 0-4 make three trips of the 256-byte-block loop (the
            # unrolled pair plus the remainder), the others two, and the
            # byte-per-lane tail kernel gets 17 bytes
            return (2 * 16384 + 5) * 256 + 17
        if ab == 8:
            return 4 * WRAP
        return WRAP * ab // 8
    return int(shape)  # sub-byte tails: an explicit byte count


UNPACK_SHAPES = ([(b, "small") for b in FORMATS] +
                 [(b, nb) for b in (1, 2, 4) for nb in (300, 255, 256 + 17)] +
                 [(b, "wrap") for b in FORMATS])


@pytest.mark.parametrize("windowed", [False, True], ids=["plain", "hamming"])
@pytest.mark.parametrize("nbits,shape", UNPACK_SHAPES)
def test_unpack_exact(C, nbits, shape, windowed):
    nbytes = raw_bytes_for(nbits, shape)
    raw = random_bytes(nbytes, seed=1000 + 7 * abs(nbits) + (nbits < 0),
                       plant=plant_for(nbits))
    count = nbytes * 8 // abs(nbits)
    w = hamming(count) if windowed else None
    expect = ref.unpack(raw, nbits, window=w)
    assert expect.size == count and expect.dtype == np.float32
    out = C.unpack(to_gpu(raw), nbits, count,
                   to_gpu(w) if windowed else None)
    if count <= 1 << 16:
        np.testing.assert_array_equal(out.cpu().numpy(), expect)
    else:
        assert_same(out, expect, f"unpack {nbits} bits, {shape}")


def test_unpack_planted_values_round_to_nearest_even():
    """What the planted words assert, stated once: the oracle itself rounds
    the 32-bit casts to nearest even."""
    got = ref.unpack(PLANT32.view(np.uint8), 32)
    assert got.tolist() == [16777215.0, 16777216.0, 2147483648.0,
                            2147483648.0, 4294967296.0]
    got = ref.unpack(PLANT32.view(np.uint8), -32)
    assert got.tolist() == [16777215.0, 16777216.0, 2147483648.0,
                            -2147483648.0, -1.0]
    assert ref.unpack(PLANT16.view(np.uint8), -16).tolist() == [
        0.0, 32767.0, -32768.0, -1.0]


@pytest.mark.parametrize("windowed", [False, True], ids=["plain", "hamming"])
@pytest.mark.parametrize("nbits", [8, -8])
@pytest.mark.parametrize("count", [1, 2, 3, 4096 + 1, 4 * WRAP + 3])
def test_unpack_8bit_any_count(C, nbits, count, windowed):
    """The samples after the last whole 4-byte word are decoded bytewise
    (srtb-correlator hands --count through as it is)."""
    raw = random_bytes(count, seed=count % 1009 + (nbits < 0))
    w = hamming(count) if windowed else None
    expect = ref.unpack(raw, nbits, window=w)
    out = C.unpack(to_gpu(raw), nbits, count, to_gpu(w) if windowed else None)
    assert_same(out, expect, f"unpack {nbits} bits, count {count}")


STREAM_COUNTS = [1 << 10, 4 * WRAP]


@pytest.mark.parametrize("windowed", [False, True], ids=["plain", "hamming"])
@pytest.mark.parametrize("per", STREAM_COUNTS)
@pytest.mark.parametrize("kind", ["interleave", "naocpsr_snap1"])
def test_unpack_2pol_exact(C, kind, per, windowed):
    raw = random_bytes(2 * per, seed=2000 + per % 1009 + len(kind))
    w = hamming(per) if windowed else None
    oracle = (ref.unpack_interleaved_2pol if kind == "interleave"
              else ref.unpack_naocpsr_snap1)
    expect = oracle(raw, window=w)
    outs = C.unpack_2pol(to_gpu(raw), kind,
                         window=to_gpu(w) if windowed else None)
    assert len(outs) == 2
    for p, (o, e) in enumerate(zip(outs, expect)):
        assert_same(o, e, f"{kind} pol {p}, {per} per pol")


@pytest.mark.parametrize("windowed", [False, True], ids=["plain", "hamming"])
@pytest.mark.parametrize("per", STREAM_COUNTS)
@pytest.mark.parametrize("ns", [2, 4])
def test_unpack_gznupsr_exact(C, ns, per, windowed):
    raw = random_bytes(ns * per, seed=3000 + per % 1009 + ns)
    w = hamming(per) if windowed else None
    expect = ref.unpack_gznupsr_a1(raw, n_streams=ns, window=w)
    outs = C.unpack_gznupsr_a1(to_gpu(raw), ns,
                               window=to_gpu(w) if windowed else None)
    assert len(outs) == ns
    for s, (o, e) in enumerate(zip(outs, expect)):
        assert_same(o, e, f"gznupsr {ns} streams, stream {s}, {per} each")


# ---------------- B. counts that do not fit ----------------

def test_unpack_subbyte_rejects_partial_byte(C):
    raw = to_gpu(random_bytes(8, seed=1))
    for nbits, count in ((1, 13), (2, 5), (4, 3)):
        with pytest.raises(RuntimeError, match="unpack"):
            C.unpack(raw, nbits, count)
    # the launcher is still usable after the rejections
    out = C.unpack(raw, 2, 32).cpu().numpy()
    np.testing.assert_array_equal(out, ref.unpack(raw.cpu().numpy(), 2))


def test_unpack_rejects_count_beyond_input(C):
    raw = to_gpu(random_bytes(8, seed=2))
    for nbits, count in ((1, 72), (8, 9), (-16, 5), (32, 3)):
        with pytest.raises(RuntimeError, match="unpack"):
            C.unpack(raw, nbits, count)
    with pytest.raises(RuntimeError, match="window"):
        C.unpack(raw, 8, 8, to_gpu(np.ones(7, dtype=np.float32)))


@pytest.mark.parametrize("kind", ["interleave", "naocpsr_snap1"])
def test_unpack_2pol_rejects_count_not_multiple_of_4(C, kind):
    with pytest.raises(RuntimeError, match="unpack"):
        C.unpack_2pol(to_gpu(random_bytes(2 * 6, seed=3)), kind)
    with pytest.raises(RuntimeError, match="unpack"):
        C.unpack_2pol(to_gpu(random_bytes(2 * 8 + 1, seed=3)), kind)


@pytest.mark.parametrize("ns", [2, 4])
def test_unpack_gznupsr_rejects_count_not_multiple_of_4(C, ns):
    with pytest.raises(RuntimeError, match="unpack"):
        C.unpack_gznupsr_a1(to_gpu(random_bytes(ns * 6, seed=4)), ns)
    with pytest.raises(RuntimeError, match="unpack"):
        C.unpack_gznupsr_a1(to_gpu(random_bytes(ns * 8 + 1, seed=4)), ns)


# ---------------- C. build_window ----------------

WINDOW_KINDS = {0: "rectangle", 1: "hann", 2: "hamming"}


@pytest.mark.parametrize("kind", [0, 1, 2])
@pytest.mark.parametrize("n", [1, 2, 5, 4096, WRAP])
def test_build_window(C, n, kind):
    """|gpu - ref| <= 2^-24 |ref| + 2^-46: float32 rounding of the value, and
    fp64 rounding of an angle of at most 2 pi times a1 <= 0.5, with room to
    spare."""
    want = ref.window_coefficients(WINDOW_KINDS[kind], n, dtype=np.float64)
    got_t = C.build_window(n, kind)
    assert got_t.dtype == torch.float32 and tuple(got_t.shape) == (n,)
    got = got_t.cpu().numpy().astype(np.float64)
    bound = U * np.abs(want) + 2.0 ** -46
    err = np.abs(got - want)
    worst = int(np.argmax(err - bound))
    print(f"WINDOW n {n} kind {kind} max err {err.max():.3e} "
          f"worst margin at {worst}: {err[worst]:.3e} vs {bound[worst]:.3e}")
    assert (err <= bound).all(), (worst, got[worst], want[worst])
    if kind == 0:
        assert (got == 1.0).all()
    if kind == 1:
        assert got[0] == 0.0
    sym = np.abs(got - got[::-1])
    assert (sym <= bound).all(), int(np.argmax(sym - bound))


def test_build_window_rejects_unknown_kind(C):
    with pytest.raises(RuntimeError, match="build_window"):
        C.build_window(16, 3)


# ---------------- D. decode at load ----------------

# first-pass kernel -> (m = n / 2, environment).  The planner
# (NativeFft::plan) was read for each row; it reports no factors, so this is
# by reading, not by assertion:
#   m = 2^13, SRTB_FFT_FACTORS=2,16,256: the override is taken as it is.
#   m = 2^14: the final pass is 64 (t >= 14), rest = 8 bits.  MAXCOL=4 gives
#     ceil(8 / 2) = 4 columns of 4; MAXCOL=8 gives 3 columns [8, 8, 4];
#     the default (64) gives 2 columns [16, 16].
#   m = 2^13: t = 13 keeps the final 256, rest = 5 bits, one column of 32:
#     the lane-pair kernel, or the mono one under SRTB_FFT_PAIR32=0.
#   m = 2^17: final 64, rest = 11 bits, two columns [64, 32]: pair64 first.
FIRST_PASS = {
    2: (1 << 13, {"SRTB_FFT_FACTORS": "2,16,256"}),
    4: (1 << 14, {"SRTB_FFT_MAXCOL": "4"}),
    8: (1 << 14, {"SRTB_FFT_MAXCOL": "8"}),
    16: (1 << 14, {}),
    32: (1 << 13, {}),
    64: (1 << 17, {}),
}


def worst(out, want):
    """max_k |out - want| / rms(want), test_gpu_fft_accuracy.py's measure for
    one row."""
    err = np.abs(out.astype(np.complex128) - want).max()
    return float(err / np.sqrt((np.abs(want) ** 2).mean()))


def decode_blocks(nbits, m):
    """(label, raw bytes) of the blocks one case transforms."""
    nbytes = 2 * m * abs(nbits) // 8
    blocks = [("random", random_bytes(nbytes, seed=4000 + abs(nbits) + m % 1009,
                                      plant=PLANT16))]
    if abs(nbits) < 8:
        # one set field in an empty block: a field read at the wrong bit
        # offset moves the impulse by a sample, an error of order 1
        at = (0x55555 % nbytes) | 1
        for v in (0x01, 0x40, 0x80):
            raw = np.zeros(nbytes, dtype=np.uint8)
            raw[at] = v
            blocks.append((f"impulse {v:#04x}", raw))
    return blocks


def check_decode(C, nbits, m, tag):
    """Both assertions of part D for one format at one plan; the plan is
    whatever the environment selects at the time of the call."""
    for label, raw in decode_blocks(nbits, m):
        raw_t = to_gpu(raw)
        fused = C.native_rfft_raw(raw_t, nbits)
        samples = C.unpack(raw_t, nbits, 2 * m)
        plain = C.native_rfft(samples)
        roc = torch.fft.rfft(samples)[:-1].cpu().numpy()
        assert tuple(fused.shape) == (m,) and fused.dtype == torch.complex64
        same = torch.equal(torch.view_as_real(fused),
                           torch.view_as_real(plain))
        x = ref.unpack(raw, nbits)
        np.testing.assert_array_equal(samples.cpu().numpy(), x)
        want = np.fft.rfft(x.astype(np.float64))[:-1]
        e_nat, e_roc = worst(fused.cpu().numpy(), want), worst(roc, want)
        diff = worst(fused.cpu().numpy(),
                     plain.cpu().numpy().astype(np.complex128))
        print(f"DECODE{tag} bits {nbits} m {m} {label} identical {same} "
              f"diff {diff:.3e} e_native {e_nat:.3e} e_roc {e_roc:.3e} "
              f"limit {2 * e_roc + 4 * U:.3e}")
        assert same, (label, "decode at load differs from unpack + FFT", diff)
        assert e_nat <= 2 * e_roc + 4 * U, (label, e_nat, e_roc)


@pytest.mark.parametrize("r2c_final", [True, False],
                         ids=["r2c_final", "r2c_post"])
@pytest.mark.parametrize("first", sorted(FIRST_PASS))
@pytest.mark.parametrize("nbits", DECODE_FORMATS)
def test_decode_at_load(C, monkeypatch, nbits, first, r2c_final):
    m, env = FIRST_PASS[first]
    for k in ("SRTB_FFT_FACTORS", "SRTB_FFT_MAXCOL", "SRTB_FFT_FINAL",
              "SRTB_FFT_R2C_FINAL"):
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    if not r2c_final:
        monkeypatch.setenv("SRTB_FFT_R2C_FINAL", "0")
    check_decode(C, nbits, m, f" N {first} r2c_final {int(r2c_final)}")


def test_native_rfft_raw_needs_a_column_first_pass(C):
    """Up to 2^12 complex elements the plan is one LDS pass, which cannot
    decode."""
    with pytest.raises(RuntimeError, match="column first pass"):
        C.native_rfft_raw(to_gpu(random_bytes(1 << 12, seed=5)), 8)
    with pytest.raises(RuntimeError, match="nbits"):
        C.native_rfft_raw(to_gpu(random_bytes(1 << 16, seed=5)), 32)


# ---------------- E. mono N = 32 column kernel ----------------

def mono32_child():
    """Runs in a process started with SRTB_FFT_PAIR32=0: one line per case,
    exit status 1 on the first failure."""
    import test_gpu_fft_accuracy as acc
    from srtb_amd.ops import native
    torch.cuda.set_device(0)
    Cn = native()
    m, _ = FIRST_PASS[32]
    try:
        for sign in (-1, 1):
            acc.check(Cn, m, sign, 7, tag=" pair32=0")
        for r2c_final in ("1", "0"):
            os.environ["SRTB_FFT_R2C_FINAL"] = r2c_final
            for nbits in DECODE_FORMATS:
                check_decode(Cn, nbits, m,
                             f" mono32 r2c_final {r2c_final}")
    except AssertionError as e:
        print("FAILED:", e)
        return 1
    print("mono32 OK")
    return 0


def test_mono32_column_kernel():
    """k_fft_col<32>, the SRTB_FFT_PAIR32=0 fallback: the plain transform at
    2^13 (both signs, batch 7) against complex128, and part D's N = 32 row."""
    env = dict(os.environ)
    for k in ("SRTB_FFT_FACTORS", "SRTB_FFT_MAXCOL", "SRTB_FFT_FINAL",
              "SRTB_FFT_R2C_FINAL"):
        env.pop(k, None)
    env["SRTB_FFT_PAIR32"] = "0"
    out = subprocess.run([sys.executable, os.path.abspath(__file__)],
                         capture_output=True, text=True, timeout=300,
                         cwd=ROOT, env=env)
    print(out.stdout[-6000:])
    assert out.returncode == 0, (out.stdout[-3000:], out.stderr[-3000:])
    lines = out.stdout.splitlines()
    assert lines[-1] == "mono32 OK"
    assert sum(l.startswith("FFTACC") for l in lines) == 2
    assert sum(l.startswith("DECODE") and "random" in l for l in lines) == 14


# ---------------- F. samples path with a window ----------------

def test_engine_samples_with_window(C):
    """submit_samples starts at the FFT: the caller multiplies by the window
    (here at unpack), the engine de-applies the waterfall window."""
    from test_gpu_engine import make_engine, small_cfg
    from srtb_amd.pipeline.cpu import CpuPipeline

    cfg = small_cfg()
    n = cfg.baseband_input_count
    rng = np.random.default_rng(29)
    raw = np.clip(np.round(rng.normal(0, 16, 2 * n)),
                  -128, 127).astype(np.int8).view(np.uint8)
    pol0 = ref.unpack_naocpsr_snap1(raw)[0].astype(np.int8).view(np.uint8)
    pipe = CpuPipeline(cfg)
    pipe.window_kind = "hamming"
    res_cpu = pipe.process_block(pol0)

    samples = C.unpack_2pol(to_gpu(raw), "naocpsr_snap1",
                            window=C.build_window(n, 2))[0]
    eng = make_engine(C, cfg, window_kind=2)
    slot = eng.submit_samples(samples)
    eng.wait(slot)
    ts_gpu = eng.time_series(slot).cpu().numpy()
    ts_cpu = res_cpu["time_series"]
    assert ts_gpu.shape == ts_cpu.shape
    scale = max(np.abs(ts_cpu).max(), 1e-9)
    np.testing.assert_allclose(ts_gpu / scale, ts_cpu / scale, atol=2e-3)


if __name__ == "__main__":
    sys.exit(mono32_child())
