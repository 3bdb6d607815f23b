"""Full-Stokes filterbank output without a GPU: the polarization-product
oracle, the nifs-aware writer and reader, the ``filterbank_polarization`` key
in Python and in the native dry-run, and ``srtb_amd.main --device cpu`` on a
two-polarization recording.  Definition: docs/ARCHITECTURE.md, "Polarization
products"."""

import glob
import os
import subprocess

import numpy as np
import pytest

from srtb_amd import ref
from srtb_amd.config import Config, parse_args, parse_config_file
from srtb_amd.io.writers import (FilterbankWriter, filterbank_header,
                                 read_filterbank)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "bin", "srtb-backend")

S, L = 8, 16


def hand_waterfalls():
    """Two [8][16] small-integer waterfalls without symmetry between them."""
    t = np.arange(L)[None, :]
    r = np.arange(S)[:, None]
    a = ((t * 7 + r * 3) % 31 - 15) + 1j * ((t * 5 + r * 11) % 29 - 14)
    b = ((t * 3 + r * 13) % 23 - 11) + 1j * ((t * 11 + r * 5) % 19 - 9)
    return a.astype(np.complex64), b.astype(np.complex64)


def cell_sums(a, b, tscrunch, fscrunch, reverse, flagged=()):
    """AA, BB, CR, CI per cell by explicit loops: [R][4][C] float64."""
    R, C = L // tscrunch, S // fscrunch
    out = np.zeros((R, 4, C))
    for c in range(C):
        row0 = S - (c + 1) * fscrunch if reverse else c * fscrunch
        for r in range(R):
            for row in range(row0, row0 + fscrunch):
                if row in flagged:
                    continue
                for t in range(r * tscrunch, (r + 1) * tscrunch):
                    x, y = float(a[row, t].real), float(a[row, t].imag)
                    u, v = float(b[row, t].real), float(b[row, t].imag)
                    out[r, 0, c] += x * x + y * y
                    out[r, 1, c] += u * u + v * v
                    out[r, 2, c] += x * u + y * v
                    out[r, 3, c] += y * u - x * v
    return out


# ---- 1. oracle ----

def test_pol_states():
    assert ref.POL_STATES == {"I": 0, "AABBCRCI": 1, "IQUV": 2}
    assert ref.POL_STATE_NIFS == {"I": 1, "AABBCRCI": 4, "IQUV": 4}


@pytest.mark.parametrize("reverse", [False, True])
@pytest.mark.parametrize("tscrunch,fscrunch", [(1, 1), (2, 4), (16, 8)])
def test_oracle_every_product_of_every_cell(tscrunch, fscrunch, reverse):
    a, b = hand_waterfalls()
    want = cell_sums(a, b, tscrunch, fscrunch, reverse)
    got = ref.pol_products_block(a, b, L, tscrunch, fscrunch, reverse,
                                 "AABBCRCI")
    assert got.dtype == np.float64
    assert got.shape == (L // tscrunch, 4, S // fscrunch)
    assert got.flags["C_CONTIGUOUS"]
    assert np.array_equal(got, want)
    # the state may be given by index, too
    assert np.array_equal(
        ref.pol_products_block(a, b, L, tscrunch, fscrunch, reverse, 1), want)
    iquv = ref.pol_products_block(a, b, L, tscrunch, fscrunch, reverse, "IQUV")
    aa, bb, cr, ci = (want[:, p] for p in range(4))
    assert np.array_equal(iquv[:, 0], aa + bb)
    assert np.array_equal(iquv[:, 1], aa - bb)
    assert np.array_equal(iquv[:, 2], 2 * cr)
    assert np.array_equal(iquv[:, 3], 2 * ci)
    i_only = ref.pol_products_block(a, b, L, tscrunch, fscrunch, reverse, "I")
    assert i_only.shape == (L // tscrunch, 1, S // fscrunch)
    assert np.array_equal(i_only[:, 0], aa + bb)
    # without flags, I is the sum of the two per-stream filterbank planes
    assert np.array_equal(
        i_only[:, 0],
        ref.filterbank_block(a, L, tscrunch, fscrunch, reverse)
        + ref.filterbank_block(b, L, tscrunch, fscrunch, reverse))


def test_oracle_valid_rows_cut_the_tail():
    a, b = hand_waterfalls()
    got = ref.pol_products_block(a, b, 13, 4, 2, False, "AABBCRCI")
    assert got.shape == (3, 4, 4)
    assert np.array_equal(got, cell_sums(a, b, 4, 2, False)[:3])


@pytest.mark.parametrize("reverse", [False, True])
def test_oracle_flag_rule(reverse):
    """A row flagged in A only contributes nothing to BB either."""
    a, b = hand_waterfalls()
    fa = np.zeros(S, dtype=np.uint8)
    fa[2] = 1
    fb = np.zeros(S, dtype=np.uint8)
    fb[5] = 1
    for flags_a, flags_b, flagged in [(fa, None, {2}), (None, fb, {5}),
                                      (fa, fb, {2, 5})]:
        got = ref.pol_products_block(a, b, L, 2, 4, reverse, "AABBCRCI",
                                     flags_a=flags_a, flags_b=flags_b)
        assert np.array_equal(got, cell_sums(a, b, 2, 4, reverse, flagged))
    one = ref.pol_products_block(a, b, L, 2, 1, False, "AABBCRCI", flags_a=fa)
    assert (one[:, :, 2] == 0).all()  # BB of the row flagged in A only
    full = ref.pol_products_block(a, b, L, 2, 1, False, "AABBCRCI")
    assert (full[:, 1, 2] > 0).all()
    assert np.array_equal(np.delete(one, 2, axis=2), np.delete(full, 2, axis=2))
    # boolean flags work as well
    assert np.array_equal(
        ref.pol_products_block(a, b, L, 2, 1, False, "AABBCRCI",
                               flags_a=fa.astype(bool)), one)


def test_oracle_identities():
    a, _ = hand_waterfalls()

    def iquv(b):
        p = ref.pol_products_block(a, b.astype(np.complex64), L, 2, 4, False,
                                   "IQUV")
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


def test_oracle_rejects_bad_input():
    a, b = hand_waterfalls()
    for args in [(L, 2, 3, False, "IQUV"),       # fscrunch does not divide S
                 (L + 1, 2, 1, False, "IQUV"),   # more valid rows than columns
                 (1, 2, 1, False, "IQUV"),       # fewer than one output row
                 (L, 0, 1, False, "IQUV"),
                 (L, 2, 1, False, "XY"),         # unknown state
                 (L, 2, 1, False, 3)]:
        with pytest.raises(ValueError):
            ref.pol_products_block(a, b, *args)
    with pytest.raises(ValueError):  # mismatched shapes
        ref.pol_products_block(a, b[:, :8], 8, 2, 1, False, "IQUV")
    with pytest.raises(ValueError):
        ref.pol_products_block(a, b, L, 2, 1, False, "IQUV",
                               flags_a=np.zeros(S + 1, dtype=np.uint8))


# ---- 2. writer and reader ----

HEADER_KW = dict(fch1=1463.5, foff=-1.0, nchans=5, tsamp=1e-4, tstart=60000.5)


@pytest.mark.parametrize("nbits", [8, 32])
def test_writer_reader_round_trip_nifs4(tmp_path, nbits):
    dtype = np.uint8 if nbits == 8 else np.float32
    rng = np.random.default_rng(nbits)
    blocks = [rng.integers(0, 200, (rows, 4, 5)).astype(dtype)
              for rows in (3, 2)]
    kw = dict(HEADER_KW, nbits=nbits, nifs=4)
    path = tmp_path / "p.fil"
    with FilterbankWriter(str(path), kw) as w:
        for blk in blocks:
            w.append(blk)
        assert w.rows == 5
        with pytest.raises(ValueError):  # the nifs = 1 shape
            w.append(blocks[0][:, 0, :])
        with pytest.raises(ValueError):
            w.append(np.zeros((3, 2, 5), dtype=dtype))
    header = filterbank_header(**kw)
    blob = path.read_bytes()
    assert blob == header + blocks[0].tobytes() + blocks[1].tobytes()
    h, data = read_filterbank(str(path))
    assert h["nifs"] == 4 and h["nbits"] == nbits and h["nchans"] == 5
    assert data.shape == (5, 4, 5) and data.dtype == dtype
    assert np.array_equal(data, np.concatenate(blocks))


@pytest.mark.parametrize("nbits", [8, 32])
def test_nifs1_files_stay_as_they_are(tmp_path, nbits):
    dtype = np.uint8 if nbits == 8 else np.float32
    block = np.arange(15).reshape(3, 5).astype(dtype)
    kw = dict(HEADER_KW, nbits=nbits)
    # the header of a file without the key says nifs = 1, byte for byte
    assert filterbank_header(**kw) == filterbank_header(**kw, nifs=1)
    blobs = []
    for i, extra in enumerate([{}, {"nifs": 1}]):
        path = tmp_path / f"one{i}.fil"
        with FilterbankWriter(str(path), dict(kw, **extra)) as w:
            w.append(block)
            with pytest.raises(ValueError):
                w.append(block[:, None, :])
        blobs.append(path.read_bytes())
        h, data = read_filterbank(str(path))
        assert h["nifs"] == 1 and data.shape == (3, 5)
        assert np.array_equal(data, block)
    assert blobs[0] == blobs[1] == filterbank_header(**kw) + block.tobytes()


# ---- 3. configuration ----

def test_python_config_key(tmp_path):
    assert Config().filterbank_polarization == ""
    for value in ("I", "AABBCRCI", "IQUV"):
        cfg = parse_args(["--filterbank_polarization", value])
        assert cfg.filterbank_polarization == value
        assert value in ref.POL_STATES
    path = tmp_path / "c.cfg"
    path.write_text("filterbank_polarization = IQUV  # all four\n")
    assert parse_config_file(str(path)).filterbank_polarization == "IQUV"
    assert parse_args(["--filterbank_polarization="]
                      ).filterbank_polarization == ""
    for bad in ("iquv", "XY", "4"):
        with pytest.raises(ValueError, match="filterbank_polarization"):
            parse_args(["--filterbank_polarization", bad])


def test_main_rejects_unusable_polarization_configs(tmp_path):
    from srtb_amd.main import main
    from tests.test_filterbank_cpu import TWO_POL_ARGS
    rec = tmp_path / "rec.bin"
    np.zeros(1 << 17, dtype=np.uint8).tofile(rec)
    base = TWO_POL_ARGS + ["--device", "cpu", "--input_file_path", str(rec),
                           "--filterbank_polarization", "IQUV"]
    out = ["--filterbank_output_path", str(tmp_path / "o.fil")]

    def exit_of(args):
        with pytest.raises(SystemExit) as e:
            main(args)
        assert e.value.code not in (0, None)
        return str(e.value.code)

    msg = exit_of(base)  # no output path
    assert "filterbank_polarization" in msg
    assert "filterbank_output_path" in msg
    msg = exit_of(base + out + ["--baseband_format_type", "simple"])
    assert "filterbank_polarization" in msg and "two data streams" in msg
    msg = exit_of(base + out + ["--dm_trial_list", "0, 40"])
    assert "dm_trial_list" in msg
    assert not os.path.exists(tmp_path / "o.fil")


def test_filterbank_paths_in_pol_mode():
    from srtb_amd.main import filterbank_header_kwargs, filterbank_paths
    cfg = Config()
    cfg.filterbank_output_path = "/data/run.1/obs.fil"
    cfg.filterbank_polarization = "IQUV"
    assert filterbank_paths(cfg, 2, 0, 1) == ["/data/run.1/obs.fil"]
    assert filterbank_paths(cfg, 2, 3, 8) == ["/data/run.1/obs_r3.fil"]
    assert filterbank_paths(cfg, 2, 3, 8, endpoint=1) == [
        "/data/run.1/obs_r3_e1.fil"]
    assert filterbank_header_kwargs(cfg)["nifs"] == 4
    cfg.filterbank_polarization = "I"
    assert filterbank_header_kwargs(cfg)["nifs"] == 1
    cfg.filterbank_polarization = ""
    assert "nifs" not in filterbank_header_kwargs(cfg)


# ---- 4. srtb_amd.main on the CPU ----

TSCRUNCH, FSCRUNCH = 4, 1
N2, S2 = 1 << 16, 64


def check_stokes_file(tmp_path, name="pol.fil"):
    """Exactly one file, [2R][4][C]; the pulse of block 1 is bright in I and
    no Stokes parameter exceeds I."""
    files = sorted(glob.glob(str(tmp_path / "pol*.fil")))
    assert files == [str(tmp_path / name)], files
    header, data = read_filterbank(files[0])
    R = N2 // (2 * S2 * TSCRUNCH)
    assert header["nifs"] == 4 and header["nbits"] == 32
    assert header["nchans"] == S2
    assert data.shape == (2 * R, 4, S2) and data.dtype == np.float32
    x = data.astype(np.float64)
    i = x[:, 0]
    row = int(np.argmax(i.sum(axis=1)))
    want = (N2 + (N2 >> 1)) // (2 * S2 * TSCRUNCH)
    assert abs(row - want) <= 1, (row, want)
    rest = np.delete(i.sum(axis=1), [row - 1, row, row + 1])
    assert i[row].sum() > rest.mean() + 6 * rest.std()
    # Cauchy-Schwarz: exact in exact arithmetic; the slack covers the fp32
    # roundings of a cell of t * f terms
    slack = (TSCRUNCH * FSCRUNCH + 3) * 2.0 ** -23 * i
    assert (i > 0).all()
    for k in (1, 2, 3):
        assert (np.abs(x[:, k]) <= i + slack).all(), k
    return header, data


def test_main_cpu_two_pol_iquv(tmp_path):
    from srtb_amd.main import main
    from tests.test_filterbank_cpu import TWO_POL_ARGS
    from tests.test_main_app import make_2pol_recording
    _, rec = make_2pol_recording(tmp_path)
    rc = main(TWO_POL_ARGS + [
        "--device", "cpu", "--input_file_path", rec,
        "--filterbank_output_path", str(tmp_path / "pol.fil"),
        "--filterbank_polarization", "IQUV", "--filterbank_nbits", "32",
        "--baseband_output_file_prefix", str(tmp_path) + "/p2_"])
    assert rc == 0
    _, data = check_stokes_file(tmp_path)
    # both streams carry the same pulse in independent noise: U > 0 there
    row = int(np.argmax(data[:, 0].astype(np.float64).sum(axis=1)))
    assert data[row, 2].astype(np.float64).sum() > 0


def test_main_cpu_two_pol_intensity_8bit(tmp_path):
    """I at 8 bits: one nifs = 1 file whose float twin is the sum of the two
    per-stream files of the default mode."""
    from srtb_amd.main import main
    from tests.test_filterbank_cpu import TWO_POL_ARGS, check_two_pol_files
    from tests.test_main_app import make_2pol_recording
    _, rec = make_2pol_recording(tmp_path)
    common = TWO_POL_ARGS + ["--device", "cpu", "--input_file_path", rec,
                             "--baseband_output_file_prefix",
                             str(tmp_path) + "/p2_"]
    (tmp_path / "sum").mkdir()
    assert main(common + ["--filterbank_output_path",
                          str(tmp_path / "sum" / "i.fil"),
                          "--filterbank_polarization", "I"]) == 0
    assert main(common + ["--filterbank_output_path",
                          str(tmp_path / "pol.fil")]) == 0
    planes = check_two_pol_files(tmp_path)
    header, total = read_filterbank(str(tmp_path / "sum" / "i.fil"))
    assert header["nifs"] == 1 and total.shape == planes[0].shape
    np.testing.assert_allclose(total, planes[0].astype(np.float64) + planes[1],
                               rtol=2.0 ** -22, atol=0)
    (tmp_path / "q").mkdir()
    assert main(common + ["--filterbank_output_path",
                          str(tmp_path / "q" / "i8.fil"),
                          "--filterbank_polarization", "I",
                          "--filterbank_nbits", "8"]) == 0
    header, q = read_filterbank(str(tmp_path / "q" / "i8.fil"))
    assert header["nbits"] == 8 and q.dtype == np.uint8
    assert q.shape == total.shape
    R = q.shape[0] // 2
    for b in range(2):
        m = q[b * R:(b + 1) * R].astype(np.float64).mean(axis=0)
        assert np.abs(m - 64).max() < 1.5, (b, m)


# ---- 5. native dry-run ----

def dry_run(*args):
    return subprocess.run([BIN, "--dry-run", *args], capture_output=True,
                          text=True, timeout=60)


needs_bin = pytest.mark.skipif(not os.path.exists(BIN),
                               reason="native binaries not built")


@needs_bin
def test_native_dry_run_echoes_the_key_only_when_set():
    out = dry_run()
    assert out.returncode == 0, out.stderr
    assert "filterbank" not in out.stdout
    out = dry_run("--filterbank_output_path", "/tmp/a.fil",
                  "--baseband_format_type", "naocpsr_snap1")
    assert out.returncode == 0, out.stderr
    assert "filterbank_polarization" not in out.stdout
    for value in ("I", "AABBCRCI", "IQUV"):
        out = dry_run("--filterbank_output_path", "/tmp/a.fil",
                      "--baseband_format_type", "naocpsr_snap1",
                      "--filterbank_polarization", value)
        assert out.returncode == 0, out.stderr
        assert f"filterbank_polarization = {value}\n" in out.stdout


@needs_bin
def test_native_rejects_unusable_polarization_configs():
    two = ["--baseband_format_type", "gznupsr_a1"]
    path = ["--filterbank_output_path", "/tmp/a.fil"]
    key = ["--filterbank_polarization", "IQUV"]
    for args, word in [
            (path + key, "two data streams"),             # single stream
            (two + key, "filterbank_output_path"),
            (two + path + key + ["--dm_trial_list", "0, 60"], "dm_trial_list"),
            (two + path + ["--filterbank_polarization", "XY"], "XY")]:
        out = dry_run(*args)
        assert out.returncode != 0, args
        text = out.stderr + out.stdout
        assert "filterbank_polarization" in text or word == "dm_trial_list"
        assert word in text, (args, text)
