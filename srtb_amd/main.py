"""srtb_amd main application — the reference `simple-radio-telescope-backend`
executable equivalent (reference src/main.cpp:61-333).

Reads a srtb_config.cfg-compatible config (cmd > cfg-file > defaults), sets up
the per-stream pipelines (native GPU engine, or the NumPy path on CPU-only
hosts), consumes baseband from a recorded file (with dedispersion-overlap
seek-back) or UDP, writes detection products (.bin/.npy/.tim) with the
polarization-coincidence scheduler, and optionally dumps live waterfall
frames (headless PPM — the Qt GUI equivalent).

Multi-GPU: launch under torchrun, one rank per GPU; streams are sharded
round-robin (parallel.sharding) and detection stats all-reduced over
RCCL/xGMI.

Usage:
  python -m srtb_amd.main --config_file_name srtb_config.cfg [--key value ...]
  torchrun --nproc-per-node 8 -m srtb_amd.main --config_file_name ...
"""

from __future__ import annotations

import sys
import time

import numpy as np

from . import ref
from .config import Config, parse_args
from .io import backends as bk
from .io.file_input import FileBlockReader
from .io.writers import (FOLD_ROW_ORDER, BlockProducts, FilterbankWriter,
                         SignalWriteScheduler, write_fold_subint)
from .pipeline.cpu import CpuPipeline
from .parallel.sharding import (DetectionAggregator, broadcast_config,
                                init_distributed, shard_streams)

# extra, non-reference options handled by the runner itself
RUNNER_FLAGS = {"--max-blocks", "--device", "--waterfall-ppm", "--gui-port",
                "--gui-linger"}


def write_ppm(path: str, argb: np.ndarray) -> None:
    """Dump an ARGB32 [H][W] image as binary PPM (P6)."""
    h, w = argb.shape
    rgb = np.empty((h, w, 3), dtype=np.uint8)
    rgb[..., 0] = (argb >> 16) & 0xFF
    rgb[..., 1] = (argb >> 8) & 0xFF
    rgb[..., 2] = argb & 0xFF
    with open(path, "wb") as f:
        f.write(b"P6\n%d %d\n255\n" % (w, h))
        f.write(rgb.tobytes())


def filterbank_plane_on(cfg: Config) -> bool:
    """Whether the blocks build the filterbank power plane: for the file, for
    the incoherent DM-offset search, or for both."""
    return bool(cfg.filterbank_output_path
                or cfg.incoherent_dm_offsets.strip())


def filterbank_time_multiple(cfg: Config) -> int:
    """The overlap's extra rounding factor: tscrunch while the filterbank
    plane is on, so a block's valid waterfall columns are whole output rows."""
    return cfg.filterbank_tscrunch if filterbank_plane_on(cfg) else 1


def filterbank_paths(cfg: Config, n_streams: int, rank: int, world: int,
                     endpoint: int | None = None) -> list[str]:
    """One output file per data stream: ``_s{k}`` goes before the extension
    for multi-stream formats, ``_r{rank}`` when several ranks run, ``_e{i}``
    when one rank serves several UDP endpoints."""
    path = cfg.filterbank_output_path
    dot = path.rfind(".")
    if dot <= path.rfind("/"):
        dot = len(path)
    stem, ext = path[:dot], path[dot:]
    tag = f"_r{rank}" if world > 1 else ""
    if endpoint is not None:
        tag += f"_e{endpoint}"
    if cfg.filterbank_polarization:
        # one file of polarization products from both streams: no ``_s{k}``
        return [stem + tag + ext]
    return [stem + (f"_s{k}" if n_streams > 1 else "") + tag + ext
            for k in range(n_streams)]


def filterbank_header_kwargs(cfg: Config) -> dict:
    kw = ref.filterbank_header_fields(
        cfg.baseband_freq_low, cfg.baseband_bandwidth,
        cfg.baseband_sample_rate, cfg.spectrum_channel_count,
        cfg.filterbank_tscrunch, cfg.filterbank_fscrunch)
    kw.update(nbits=cfg.filterbank_nbits, tstart=cfg.filterbank_tstart_mjd)
    if cfg.filterbank_polarization:
        kw.update(nifs=ref.POL_STATE_NIFS[cfg.filterbank_polarization])
    return kw


def check_filterbank_polarization(cfg: Config, n_streams: int) -> None:
    """Reject a filterbank_polarization the run cannot honour."""
    if not cfg.filterbank_polarization:
        return
    if not cfg.filterbank_output_path:
        raise SystemExit(
            "config: filterbank_polarization needs filterbank_output_path")
    if n_streams != 2:
        raise SystemExit(
            "config: filterbank_polarization needs a baseband_format_type "
            f"with exactly two data streams ({cfg.baseband_format_type!r} "
            f"has {n_streams})")
    if cfg.dm_trial_list.strip():
        raise SystemExit(
            "config: filterbank_polarization and dm_trial_list exclude each "
            "other (a filterbank file holds one DM)")


def check_incoherent_config(cfg: Config) -> None:
    """Reject an incoherent_dm_offsets the run cannot honour."""
    if not 1 <= cfg.incoherent_normalize_blocks <= ref.INCOH_NORM_MAX_BLOCKS:
        raise SystemExit(
            "config: incoherent_normalize_blocks must be 1 .. "
            f"{ref.INCOH_NORM_MAX_BLOCKS}")
    if not cfg.incoherent_dm_offsets.strip():
        if cfg.incoherent_output_path:
            raise SystemExit(
                "config: incoherent_output_path needs incoherent_dm_offsets")
        if cfg.incoherent_normalize:
            raise SystemExit(
                "config: incoherent_normalize needs incoherent_dm_offsets")
        return
    if not cfg.incoherent_output_path:
        raise SystemExit(
            "config: incoherent_dm_offsets needs incoherent_output_path")
    if cfg.dm_trial_list.strip():
        raise SystemExit(
            "config: incoherent_dm_offsets and dm_trial_list exclude each "
            "other (the offsets are searched around the one coherent dm)")
    if cfg.filterbank_polarization:
        raise SystemExit(
            "config: incoherent_dm_offsets and filterbank_polarization "
            "exclude each other (the search runs on per-stream planes)")


def incoherent_paths(cfg: Config, n_streams: int, rank: int, world: int,
                     endpoint: int | None = None) -> list[str]:
    """One candidates file per data stream, tagged like the filterbank's."""
    fil = cfg.copy()
    fil.filterbank_output_path = cfg.incoherent_output_path
    return filterbank_paths(fil, n_streams, rank, world, endpoint)


class IncoherentOutput:
    """The searchers of one pipeline (one per data stream) and their
    candidates files.  On the GPU a searcher consumes the engine slot's power
    plane on its own stream; on the CPU it is ref.CpuIncoherentSearch fed with
    the oracle plane."""

    def __init__(self, cfg: Config, paths: list[str], rows: int,
                 native=None):
        hdr = ref.filterbank_header_fields(
            cfg.baseband_freq_low, cfg.baseband_bandwidth,
            cfg.baseband_sample_rate, cfg.spectrum_channel_count,
            cfg.filterbank_tscrunch, cfg.filterbank_fscrunch)
        self.cfg, self.tsamp = cfg, hdr["tsamp"]
        self.native = native
        kw = dict(fch1=hdr["fch1"], foff=hdr["foff"], tsamp=hdr["tsamp"],
                  offsets=cfg.incoherent_offsets(),
                  snr_threshold=cfg.signal_detect_signal_noise_threshold,
                  max_boxcar=cfg.signal_detect_max_boxcar_length)
        if cfg.incoherent_normalize:  # off: the searchers' own defaults
            kw.update(normalize=True,
                      normalize_blocks=cfg.incoherent_normalize_blocks)
        try:
            if native is not None:
                self.searchers = [native.IncoherentSearch(
                    rows=rows, channels=hdr["nchans"], **kw) for _ in paths]
            else:
                self.searchers = [ref.CpuIncoherentSearch(
                    rows, hdr["nchans"], **kw) for _ in paths]
        except (RuntimeError, ValueError) as e:
            raise SystemExit(f"config: {e}")
        self.files = [open(p_, "w") for p_ in paths]

    def block_done(self, pipe) -> None:
        if self.native is not None:
            engines = getattr(pipe, "engines", None) or [pipe.eng]
            slots = getattr(pipe, "last_slots", None) or [pipe.last_slot]
            ks = [s.submit(e, sl)
                  for s, e, sl in zip(self.searchers, engines, slots)]
            results = [s.wait(k) for s, k in zip(self.searchers, ks)]
        else:
            results = [s.add(plane) for s, plane in
                       zip(self.searchers, pipe.filterbank_power_blocks())]
        for f, res in zip(self.files, results):
            f.writelines(ref.incoherent_candidate_lines(
                res, self.tsamp, self.cfg.dm))

    def reset(self) -> None:
        for s in self.searchers:
            s.reset()

    def close(self) -> None:
        for f in self.files:
            f.close()


def cpu_pol_filterbank_block(cfg: Config, results: list,
                             nsamps_reserved: int) -> np.ndarray:
    """The combiner's [R][P][C] rows of one block from the oracle functions
    (results: the two polarizations' CPU pipeline result dicts)."""
    wf_a, wf_b = results[0]["waterfall"], results[1]["waterfall"]
    valid = ref.filterbank_valid_rows(cfg.baseband_input_count, wf_a.shape[0],
                                      nsamps_reserved)
    plane = ref.pol_products_block(
        wf_a, wf_b, valid, cfg.filterbank_tscrunch, cfg.filterbank_fscrunch,
        reverse=cfg.baseband_bandwidth > 0,
        pol_state=cfg.filterbank_polarization,
        flags_a=results[0]["sk_flags"],
        flags_b=results[1]["sk_flags"]).astype(np.float32)
    if cfg.filterbank_nbits == 32:
        return plane
    flat = plane.reshape(plane.shape[0], -1)
    mean, std = ref.filterbank_channel_stats(flat)
    return ref.filterbank_quantize(flat, mean, std).reshape(plane.shape)


def cpu_filterbank_power(cfg: Config, wf: np.ndarray,
                         nsamps_reserved: int) -> np.ndarray:
    """The float32 power plane [R][C] of one block from the oracle."""
    valid = ref.filterbank_valid_rows(cfg.baseband_input_count, wf.shape[0],
                                      nsamps_reserved)
    return ref.filterbank_block(
        wf, valid, cfg.filterbank_tscrunch, cfg.filterbank_fscrunch,
        reverse=cfg.baseband_bandwidth > 0).astype(np.float32)


def cpu_filterbank_block(cfg: Config, wf: np.ndarray,
                         nsamps_reserved: int) -> np.ndarray:
    """The engine's filterbank rows of one block from the oracle functions
    (wf: the SK-zapped waterfall)."""
    power = cpu_filterbank_power(cfg, wf, nsamps_reserved)
    if cfg.filterbank_nbits == 32:
        return power
    mean, std = ref.filterbank_channel_stats(power)
    return ref.filterbank_quantize(power, mean, std)


def fold_stems(cfg: Config, n_streams: int, rank: int, world: int,
               endpoint: int | None = None) -> list[str]:
    """One file stem per data stream, tagged like the filterbank's files
    (``_s{k}``, ``_r{rank}``, ``_e{i}``); a trailing ``.npy`` of
    ``fold_output_path`` is dropped.  Sub-integration i then writes
    ``{stem}_{i:04d}.npy``, ``.hits.npy``, ``.weights.npy`` and ``.txt``."""
    stem = cfg.fold_output_path
    if stem.endswith(".npy"):
        stem = stem[:-4]
    tag = f"_r{rank}" if world > 1 else ""
    if endpoint is not None:
        tag += f"_e{endpoint}"
    return [stem + (f"_s{k}" if n_streams > 1 else "") + tag
            for k in range(n_streams)]


def check_fold_config(cfg: Config) -> None:
    """Reject a fold configuration before anything is allocated."""
    if cfg.dm_trial_list.strip():
        raise SystemExit(
            "config: fold_output_path and dm_trial_list exclude each other "
            "(a folded profile holds one DM)")
    try:
        f0, _f1 = cfg.fold_spin()
        ref.fold_check(cfg.spectrum_channel_count, cfg.baseband_sample_rate,
                       f0, cfg.fold_nbin)
    except ValueError as e:
        raise SystemExit(f"config: {e}")
    if cfg.fold_subint_blocks < 0:
        raise SystemExit("config: fold_subint_blocks must not be negative")


class FoldOutput:
    """Sub-integration bookkeeping of one pipeline: after every
    ``fold_subint_blocks`` blocks, and at the end of the run, the pipeline's
    accumulators are read, written and reset."""

    def __init__(self, cfg: Config, stems: list[str]):
        self.cfg = cfg
        self.stems = stems
        self.index = 0
        self.blocks = 0
        self.first_sample = 0

    def block_done(self, pipe, first_sample: int) -> None:
        if self.blocks == 0:
            self.first_sample = first_sample
        self.blocks += 1
        if self.cfg.fold_subint_blocks and \
                self.blocks >= self.cfg.fold_subint_blocks:
            self.flush(pipe)

    def flush(self, pipe) -> None:
        if self.blocks == 0:
            return
        cfg = self.cfg
        f0, f1 = cfg.fold_spin()
        meta = {
            "f0": f0, "f1": f1, "phase0": float(cfg.fold_phase_offset),
            "nbin": cfg.fold_nbin, "first_sample": self.first_sample,
            "n_blocks": self.blocks,
            "tsamp": 2.0 * cfg.spectrum_channel_count /
            cfg.baseband_sample_rate,
            "freq_low": float(cfg.baseband_freq_low),
            "bandwidth": float(cfg.baseband_bandwidth), "dm": float(cfg.dm),
            "row_order": FOLD_ROW_ORDER,
        }
        for stem, (acc, hits, weights) in zip(self.stems, pipe.fold_take()):
            write_fold_subint(stem, self.index, acc, hits, weights, meta)
        self.index += 1
        self.blocks = 0


def _cpu_folder(cfg: Config, nsamps_reserved: int):
    if not cfg.fold_output_path:
        return None
    f0, f1 = cfg.fold_spin()
    return ref.CpuFolder(cfg.baseband_input_count, nsamps_reserved,
                         cfg.spectrum_channel_count, cfg.baseband_sample_rate,
                         f0, f1, cfg.fold_phase_offset, cfg.fold_nbin)


def _cpu_fold_add(folder, wf: np.ndarray) -> None:
    """Fold the SK-zapped waterfall of one block; its all-zero rows are the
    flagged ones."""
    folder.add(wf, ~(wf != 0).any(axis=1))


def _cpu_fold_take(folders) -> list:
    out = [f.read() for f in folders]
    for f in folders:
        f.reset()
    return out


def _engine_fold_take(engines) -> list:
    out = [e.fold_read() for e in engines]
    for e in engines:
        e.fold_reset()
    return out


def _engine_products(eng, cfg: Config, slot: int, res: dict,
                     raw: np.ndarray | None, counter: int) -> BlockProducts:
    """Build the dumpable products of one processed block from a native
    engine slot (detection gate + waterfall/time-series extraction)."""
    # raw baseband is attached even without a detection: the reference's
    # write_signal works always carry baseband_data, so a cross-pol
    # coincidence write can dump the negative stream's baseband too
    products = BlockProducts(counter=counter, timestamp=counter, raw=raw)
    gate = res["zero_count"] < (cfg.signal_detect_channel_threshold *
                                cfg.spectrum_channel_count)
    detected = [(L, c) for L, c in res["counts"] if c > 0]
    if gate and detected:
        products.waterfall = eng.waterfall(slot).cpu().numpy()
        ts = eng.time_series(slot).cpu().numpy()
        for L, _count in detected:
            if L == 1:
                products.time_series.append((1, ts.copy()))
            else:
                products.time_series.append(
                    (L, eng.boxcar_series(slot, L).cpu().numpy()))
    return products


class GpuStreamPipeline:
    """One data stream on one GPU via the native engine."""

    def __init__(self, cfg: Config, nsamps_reserved: int):
        import torch
        from .ops import native
        from .pipeline.gpu import filterbank_engine_kwargs, fold_engine_kwargs
        self.torch = torch
        self.C = native()
        self.cfg = cfg
        ranges = ref.parse_rfi_freq_list(cfg.mitigate_rfi_freq_list)
        nc = cfg.baseband_input_count // 2
        bins = ref.rfi_ranges_to_bins(cfg.baseband_freq_low,
                                      cfg.baseband_bandwidth, nc, ranges)
        self.eng = self.C.PipelineEngine(
            n=cfg.baseband_input_count, nbits=cfg.baseband_input_bits,
            channels=cfg.spectrum_channel_count,
            freq_low=cfg.baseband_freq_low, bandwidth=cfg.baseband_bandwidth,
            sample_rate=cfg.baseband_sample_rate, dm=cfg.dm,
            rfi_threshold=cfg.mitigate_rfi_average_method_threshold,
            sk_threshold=cfg.mitigate_rfi_spectral_kurtosis_threshold,
            snr_threshold=cfg.signal_detect_signal_noise_threshold,
            max_boxcar=cfg.signal_detect_max_boxcar_length,
            nsamps_reserved=nsamps_reserved,
            zap_ranges=[[int(a), int(b)] for a, b in bins],
            use_phase_table=False, enable_rfi_s1=True, enable_sk=True,
            n_slots=2, **filterbank_engine_kwargs(cfg),
            **fold_engine_kwargs(cfg))

    def filterbank_blocks(self) -> list[np.ndarray]:
        return [self.eng.filterbank(self.last_slot).numpy()]

    def fold_position(self, n0: int) -> None:
        self.eng.set_fold_next_sample(n0)

    def fold_take(self) -> list:
        return _engine_fold_take([self.eng])

    def process_block(self, raw: np.ndarray, counter: int) -> BlockProducts:
        torch = self.torch
        t = torch.from_numpy(np.ascontiguousarray(raw))
        slot = self.eng.submit(t)
        res = self.eng.wait(slot)
        self.last_result = res
        self.last_slot = slot
        return _engine_products(self.eng, self.cfg, slot, res, raw, counter)

    def waterfall_frame(self, width: int, height: int) -> np.ndarray:
        wf = self.eng.waterfall(self.last_slot)
        img = self.C.resample_power(wf, height, width)
        self.C.normalize_by_mean(img)
        pix = self.C.generate_pixmap(img, ref.COLOR_0, ref.COLOR_1,
                                     ref.COLOR_OVERFLOW)
        return pix.cpu().numpy().view(np.uint32)

    def spectrum_lines(self) -> list[np.ndarray]:
        # per-channel mean intensity of the latest waterfall (the
        # reference's live spectrum view, src/spectrum.qml)
        wf = self.eng.waterfall(self.last_slot)
        return [(wf.real ** 2 + wf.imag ** 2).mean(dim=1).cpu().numpy()]


class GpuMultiPolPipeline:
    """One PACKED packet stream fanning out into per-polarization sample
    streams, each through its own engine (reference unpack_pipe.hpp:146-390
    fans one naocpsr_snap1 / gznupsr_a1 stream into data_stream_id works)."""

    def __init__(self, cfg: Config, nsamps_reserved: int, fmt_name: str):
        import torch
        from .ops import native
        from .pipeline.gpu import (_make_engine, filterbank_engine_kwargs,
                                   fold_engine_kwargs)
        self.torch = torch
        self.C = native()
        self.cfg = cfg
        self.fmt = bk.resolve_alias(fmt_name)
        self.n_streams = bk.get_data_stream_count(fmt_name)
        self.engines = [_make_engine(self.C, cfg, nsamps_reserved, nbits=-8,
                                     **filterbank_engine_kwargs(cfg),
                                     **fold_engine_kwargs(cfg))
                        for _ in range(self.n_streams)]
        # filterbank_polarization: the engines make no per-stream planes (the
        # keywords above are empty then); one combiner joins the two streams
        self.combiner = None
        self.combiner_slot = None
        if cfg.filterbank_polarization:
            self.combiner = self.C.PolCombiner(
                n=cfg.baseband_input_count,
                channels=cfg.spectrum_channel_count,
                nsamps_reserved=nsamps_reserved,
                tscrunch=cfg.filterbank_tscrunch,
                fscrunch=cfg.filterbank_fscrunch,
                reverse=cfg.baseband_bandwidth > 0,
                pol_state=ref.POL_STATES[cfg.filterbank_polarization],
                nbits=cfg.filterbank_nbits)

    def fold_position(self, n0: int) -> None:
        for e in self.engines:
            e.set_fold_next_sample(n0)

    def fold_take(self) -> list:
        return _engine_fold_take(self.engines)

    def filterbank_blocks(self) -> list[np.ndarray]:
        if self.combiner is not None:
            k, self.combiner_slot = self.combiner_slot, None
            self.combiner.wait(k)
            return [self.combiner.plane(k).numpy()]
        return [e.filterbank(s).numpy()
                for e, s in zip(self.engines, self.last_slots)]

    def _fanout(self, raw_t):
        if self.fmt == "gznupsr_a1":
            return self.C.unpack_gznupsr_a1(raw_t, self.n_streams)
        return self.C.unpack_2pol(raw_t, self.fmt)

    def process_blocks(self, raw: np.ndarray,
                       counter: int) -> list[BlockProducts]:
        torch = self.torch
        raw_t = torch.from_numpy(np.ascontiguousarray(raw)).cuda()
        pols = self._fanout(raw_t)
        if self.combiner_slot is not None:
            # the last plane was never fetched: the combiner still reads the
            # engines' slots until its wait returns
            self.combiner.wait(self.combiner_slot)
        slots = [eng.submit_samples(pol)
                 for eng, pol in zip(self.engines, pols)]
        if self.combiner is not None:
            self.combiner_slot = self.combiner.submit(
                self.engines[0], slots[0], self.engines[1], slots[1])
        out = []
        results = []
        for eng, slot in zip(self.engines, slots):
            res = eng.wait(slot)
            results.append(res)
            # both pols share the same raw packet block (as the reference's
            # fanned-out works share baseband_data): attach it to each so a
            # coincidence write from either stream dumps it
            out.append(_engine_products(eng, self.cfg, slot, res, raw,
                                        counter))
        self.last_result = results[0]
        self.last_slot = slots[0]
        self.last_slots = slots
        return out

    def _frame(self, eng, slot, width: int, height: int) -> np.ndarray:
        wf = eng.waterfall(slot)
        img = self.C.resample_power(wf, height, width)
        self.C.normalize_by_mean(img)
        pix = self.C.generate_pixmap(img, ref.COLOR_0, ref.COLOR_1,
                                     ref.COLOR_OVERFLOW)
        return pix.cpu().numpy().view(np.uint32)

    def waterfall_frame(self, width: int, height: int) -> np.ndarray:
        return self._frame(self.engines[0], self.last_slot, width, height)

    def waterfall_frames(self, width: int, height: int) -> list[np.ndarray]:
        """One pixmap per data stream (the reference opens one waterfall
        window per stream, src/main.qml:14-28)."""
        return [self._frame(e, s, width, height)
                for e, s in zip(self.engines, self.last_slots)]

    def spectrum_lines(self) -> list[np.ndarray]:
        out = []
        for e, sl in zip(self.engines, self.last_slots):
            wf = e.waterfall(sl)
            out.append((wf.real ** 2 + wf.imag ** 2).mean(dim=1)
                       .cpu().numpy())
        return out


class CpuMultiPolPipeline:
    """CPU/NumPy twin of GpuMultiPolPipeline (oracle + plumbing runs)."""

    def __init__(self, cfg: Config, nsamps_reserved: int, fmt_name: str):
        self.cfg = cfg
        self.fmt = bk.resolve_alias(fmt_name)
        self.n_streams = bk.get_data_stream_count(fmt_name)
        self.nsamps_reserved = nsamps_reserved
        self.pipes = [CpuPipeline(cfg, nsamps_reserved)
                      for _ in range(self.n_streams)]
        self.folders = [_cpu_folder(cfg, nsamps_reserved)
                        for _ in range(self.n_streams)]

    def fold_position(self, n0: int) -> None:
        for f in self.folders:
            f.next_sample = n0

    def fold_take(self) -> list:
        return _cpu_fold_take(self.folders)

    def filterbank_blocks(self) -> list[np.ndarray]:
        if self.cfg.filterbank_polarization:
            return [cpu_pol_filterbank_block(self.cfg, self.last_results,
                                             self.nsamps_reserved)]
        return [cpu_filterbank_block(self.cfg, r["waterfall"],
                                     self.nsamps_reserved)
                for r in self.last_results]

    def filterbank_power_blocks(self) -> list[np.ndarray]:
        return [cpu_filterbank_power(self.cfg, r["waterfall"],
                                     self.nsamps_reserved)
                for r in self.last_results]

    def _fanout(self, raw: np.ndarray) -> list[np.ndarray]:
        if self.fmt == "gznupsr_a1":
            return ref.unpack_gznupsr_a1(raw, self.n_streams)
        return list(ref.unpack_naocpsr_snap1(raw))

    def process_blocks(self, raw: np.ndarray,
                       counter: int) -> list[BlockProducts]:
        cfg = self.cfg
        out = []
        self.last_results = []
        for pipe, folder, samples in zip(self.pipes, self.folders,
                                         self._fanout(raw)):
            res = pipe.process_samples(samples)
            if folder is not None:
                _cpu_fold_add(folder, res["waterfall"])
            self.last_result = res
            self.last_results.append(res)
            products = BlockProducts(counter=counter, timestamp=counter,
                                     raw=raw)
            gate = res["zero_count"] < (cfg.signal_detect_channel_threshold *
                                        cfg.spectrum_channel_count)
            if gate and res["detections"]:
                products.waterfall = res["waterfall"]
                for L, _cnt, series in res["detections"]:
                    products.time_series.append((L, series))
            out.append(products)
        return out

    def waterfall_frame(self, width: int, height: int) -> np.ndarray:
        wf = self.last_result["waterfall"]
        p = np.abs(wf.astype(np.complex64)) ** 2
        img = ref.resample_power_2d(p, height, width)
        img = ref.normalize_by_mean(img)
        return ref.generate_pixmap(img)

    def waterfall_frames(self, width: int, height: int) -> list[np.ndarray]:
        out = []
        for res in self.last_results:
            p = np.abs(res["waterfall"].astype(np.complex64)) ** 2
            img = ref.normalize_by_mean(ref.resample_power_2d(p, height,
                                                              width))
            out.append(ref.generate_pixmap(img))
        return out

    def spectrum_lines(self) -> list[np.ndarray]:
        return [(np.abs(r["waterfall"].astype(np.complex64)) ** 2
                 ).mean(axis=1) for r in self.last_results]


class CpuStreamPipeline:
    """CPU/NumPy path (plumbing runs, no GPU)."""

    def __init__(self, cfg: Config, nsamps_reserved: int):
        self.cfg = cfg
        self.nsamps_reserved = nsamps_reserved
        self.pipe = CpuPipeline(cfg, nsamps_reserved)
        self.folder = _cpu_folder(cfg, nsamps_reserved)

    def fold_position(self, n0: int) -> None:
        self.folder.next_sample = n0

    def fold_take(self) -> list:
        return _cpu_fold_take([self.folder])

    def filterbank_blocks(self) -> list[np.ndarray]:
        return [cpu_filterbank_block(self.cfg, self.last_result["waterfall"],
                                     self.nsamps_reserved)]

    def filterbank_power_blocks(self) -> list[np.ndarray]:
        return [cpu_filterbank_power(self.cfg, self.last_result["waterfall"],
                                     self.nsamps_reserved)]

    def process_block(self, raw: np.ndarray, counter: int) -> BlockProducts:
        cfg = self.cfg
        res = self.pipe.process_block(raw)
        self.last_result = res
        if self.folder is not None:
            _cpu_fold_add(self.folder, res["waterfall"])
        products = BlockProducts(counter=counter, timestamp=counter, raw=raw)
        gate = res["zero_count"] < (cfg.signal_detect_channel_threshold *
                                    cfg.spectrum_channel_count)
        if gate and res["detections"]:
            products.waterfall = res["waterfall"]
            for L, _cnt, series in res["detections"]:
                products.time_series.append((L, series))
        return products

    def waterfall_frame(self, width: int, height: int) -> np.ndarray:
        wf = self.last_result["waterfall"]
        p = np.abs(wf.astype(np.complex64)) ** 2
        img = ref.resample_power_2d(p, height, width)
        img = ref.normalize_by_mean(img)
        return ref.generate_pixmap(img)

    def spectrum_lines(self) -> list[np.ndarray]:
        wf = self.last_result["waterfall"]
        return [(np.abs(wf.astype(np.complex64)) ** 2).mean(axis=1)]


def main(argv=None) -> int:
    argv = list(sys.argv[1:] if argv is None else argv)
    # split runner-only flags from reference-style config options
    max_blocks = None
    device = None
    waterfall_every = 0
    gui_port = 8265
    gui_linger = 0.0
    cfg_argv = []
    i = 0
    while i < len(argv):
        a = argv[i]
        if a.startswith("--max-blocks"):
            max_blocks = int(a.split("=", 1)[1] if "=" in a else argv[i + 1])
            i += 1 if "=" in a else 2
        elif a.startswith("--device"):
            device = a.split("=", 1)[1] if "=" in a else argv[i + 1]
            i += 1 if "=" in a else 2
        elif a.startswith("--waterfall-ppm"):
            waterfall_every = int(a.split("=", 1)[1] if "=" in a else argv[i + 1])
            i += 1 if "=" in a else 2
        elif a.startswith("--gui-port"):
            gui_port = int(a.split("=", 1)[1] if "=" in a else argv[i + 1])
            i += 1 if "=" in a else 2
        elif a.startswith("--gui-linger"):
            gui_linger = float(a.split("=", 1)[1] if "=" in a else argv[i + 1])
            i += 1 if "=" in a else 2
        else:
            cfg_argv.append(a)
            i += 1
    rank, world, local_rank = init_distributed()
    cfg = parse_args(cfg_argv) if rank == 0 else Config()
    cfg = broadcast_config(cfg if rank == 0 else None)

    check_incoherent_config(cfg)
    if filterbank_plane_on(cfg):
        if cfg.dm_trial_list.strip():
            raise SystemExit(
                "config: filterbank_output_path and dm_trial_list exclude each "
                "other (a filterbank file holds one DM)")
        t, f = cfg.filterbank_tscrunch, cfg.filterbank_fscrunch
        s_ = cfg.spectrum_channel_count
        if (t < 1 or t & (t - 1) or t > 4096 or f < 1 or f & (f - 1)
                or s_ % f or cfg.filterbank_nbits not in (8, 32)):
            raise SystemExit(
                "config: filterbank_tscrunch must be a power of two <= 4096, "
                "filterbank_fscrunch a power of two dividing "
                "spectrum_channel_count, filterbank_nbits 8 or 32")

    check_filterbank_polarization(
        cfg, bk.get_data_stream_count(cfg.baseband_format_type))

    fold_on = bool(cfg.fold_output_path)
    if fold_on:
        check_fold_config(cfg)

    import importlib
    torch_spec = importlib.util.find_spec("torch")
    use_gpu = False
    if device != "cpu" and torch_spec is not None:
        import torch
        use_gpu = torch.cuda.is_available()

    reserved = ref.nsamps_reserved(
        cfg.baseband_input_count, cfg.spectrum_channel_count,
        cfg.baseband_freq_low, cfg.baseband_bandwidth,
        cfg.baseband_sample_rate, cfg.dm, cfg.baseband_reserve_sample,
        time_multiple=filterbank_time_multiple(cfg))

    # polarization fan-out: formats with >1 data stream run one packed
    # packet stream through per-pol pipelines + cross-pol coincidence writes
    n_streams = bk.get_data_stream_count(cfg.baseband_format_type)

    def make(cfg_, reserved_):
        if n_streams > 1:
            cls = GpuMultiPolPipeline if use_gpu else CpuMultiPolPipeline
            return cls(cfg_, reserved_, cfg.baseband_format_type)
        return (GpuStreamPipeline if use_gpu else CpuStreamPipeline)(
            cfg_, reserved_)

    def process(pipe, raw, counter) -> list[BlockProducts]:
        if hasattr(pipe, "process_blocks"):
            return pipe.process_blocks(raw, counter)
        return [pipe.process_block(raw, counter)]

    # live waterfall GUI (reference Qt windows → built-in browser viewer);
    # only rank 0 serves when running under torchrun
    gui = None
    if cfg.gui_enable and rank == 0:
        from .gui import WaterfallServer
        gui = WaterfallServer(port=gui_port).start()
        print(f"[srtb_amd] live waterfall: http://127.0.0.1:{gui.port}/")

    def gui_update(pipe, blocks_done, written):
        if gui is None:
            return
        try:
            if hasattr(pipe, "waterfall_frames"):
                frames = pipe.waterfall_frames(cfg.gui_pixmap_width,
                                               cfg.gui_pixmap_height)
            else:
                frames = [pipe.waterfall_frame(cfg.gui_pixmap_width,
                                               cfg.gui_pixmap_height)]
        except Exception:
            return  # no block processed yet
        for sid, frame in enumerate(frames):
            gui.push_frame(sid, frame)
        try:
            for sid, line in enumerate(pipe.spectrum_lines()):
                gui.push_spectrum(sid, line)
        except Exception:
            pass
        gui.update_status(blocks=blocks_done, written=written)

    agg = DetectionAggregator()
    writer = SignalWriteScheduler(
        cfg.baseband_output_file_prefix, cfg.baseband_input_count,
        cfg.baseband_sample_rate, real_time=(cfg.input_file_path == ""),
        async_writes=True)

    # continuous filterbank output: one file per data stream (and endpoint)
    fil_writers: dict = {}

    def fil_append(pipe, ep=None, n_eps=1):
        if not cfg.filterbank_output_path:
            return
        if ep not in fil_writers:
            paths = filterbank_paths(cfg, n_streams, rank, world,
                                     endpoint=ep if n_eps > 1 else None)
            fil_writers[ep] = [FilterbankWriter(
                p_, filterbank_header_kwargs(cfg)) for p_ in paths]
        for w, rows in zip(fil_writers[ep], pipe.filterbank_blocks()):
            if rows.ndim == 3 and w.nifs == 1:
                rows = rows[:, 0, :]  # polarization state I: [R][1][C]
            w.append(rows)

    if filterbank_plane_on(cfg):
        valid = cfg.baseband_input_count - reserved
        per = 2 * cfg.spectrum_channel_count * cfg.filterbank_tscrunch
        if valid <= 0 or valid % per:
            raise SystemExit(
                f"config: baseband_input_count - overlap = {valid} is not a "
                f"positive multiple of 2 * spectrum_channel_count * "
                f"filterbank_tscrunch = {per}")

    # incoherent DM-offset search: one IncoherentOutput per pipeline (per
    # endpoint in UDP mode), one searcher and candidates file per data stream
    incoh_on = bool(cfg.incoherent_dm_offsets.strip())
    incoh_outs: dict = {}

    def incoh_block_done(pipe, ep=None, n_eps=1, dropped=False):
        if ep not in incoh_outs:
            rows = ((cfg.baseband_input_count - reserved)
                    // (2 * cfg.spectrum_channel_count
                        * cfg.filterbank_tscrunch))
            incoh_outs[ep] = IncoherentOutput(
                cfg, incoherent_paths(cfg, n_streams, rank, world,
                                      endpoint=ep if n_eps > 1 else None),
                rows, native=getattr(pipe, "C", None))
        if dropped:
            print(f"[srtb_amd] incoherent search: data was dropped before "
                  f"this block{'' if ep is None else f' of endpoint {ep}'}; "
                  f"the history restarts")
            incoh_outs[ep].reset()
        incoh_outs[ep].block_done(pipe)

    # pulsar folding: one FoldOutput per pipeline (per endpoint in UDP mode)
    fold_outs: dict = {}

    def fold_block_done(pipe, first_sample, ep=None, n_eps=1):
        if ep not in fold_outs:
            fold_outs[ep] = FoldOutput(cfg, fold_stems(
                cfg, n_streams, rank, world,
                endpoint=ep if n_eps > 1 else None))
        fold_outs[ep].block_done(pipe, first_sample)

    if fold_on:
        valid = cfg.baseband_input_count - reserved
        if valid <= 0 or valid % (2 * cfg.spectrum_channel_count):
            raise SystemExit(
                f"config: baseband_input_count - overlap = {valid} is not a "
                f"positive multiple of 2 * spectrum_channel_count (fold)")

    t0 = time.time()
    n_blocks = 0
    # baseband_write_all: record every block (minus the overlap tail) into
    # one file per stream (reference write_file_pipe.hpp:41-94)
    write_all_f = None
    if cfg.baseband_write_all:
        write_all_f = open(cfg.baseband_output_file_prefix +
                           f"all_r{rank}.bin", "ab")
        reserved_bytes = reserved * abs(cfg.baseband_input_bits) // 8

    if cfg.input_file_path:
        # file replay: one packet/sample stream (multi-pol formats carry
        # n_streams interleaved sample streams per block)
        pipe = make(cfg, reserved)
        reader = FileBlockReader(cfg.input_file_path,
                                 cfg.baseband_input_count * n_streams,
                                 cfg.baseband_input_bits, reserved * n_streams,
                                 cfg.input_file_offset_bytes)
        for sample_index, raw in reader:
            if fold_on:
                # the block's true position in its sample stream, always: a
                # replay that skips blocks then still folds in phase
                pipe.fold_position(sample_index // n_streams)
            for products in process(pipe, raw, sample_index):
                writer.push(products)
            fil_append(pipe)
            if incoh_on:
                incoh_block_done(pipe)
            if fold_on:
                fold_block_done(pipe, sample_index // n_streams)
            if write_all_f is not None:
                end = raw.size - reserved_bytes if reserved_bytes else raw.size
                write_all_f.write(raw[:end].tobytes())
            res = getattr(pipe, "last_result", None)
            if isinstance(res, dict) and "zero_count" in res:
                zc = res["zero_count"]
                counts = (res.get("counts")
                          or [(L, c) for L, c, _ in res.get("detections", [])])
            else:
                zc, counts = 0, []
            agg.update(int(zc), [(int(a), int(b)) for a, b in counts])
            n_blocks += 1
            gui_update(pipe, n_blocks, len(writer.written))
            if waterfall_every and n_blocks % waterfall_every == 0:
                frame = pipe.waterfall_frame(cfg.gui_pixmap_width,
                                             cfg.gui_pixmap_height)
                write_ppm(f"{cfg.baseband_output_file_prefix}"
                          f"waterfall_r{rank}_{n_blocks}.ppm", frame)
            if max_blocks is not None and n_blocks >= max_blocks:
                break
    else:
        # UDP ingest: endpoints sharded across ranks; each rank runs one
        # receiver thread per assigned endpoint (the reference spawns N udp
        # receiver pipes, main.cpp:230-272), feeding a shared work queue
        import queue as _queue
        import threading
        from .io.udp import BlockAssembler, UdpPacketProvider, run_receiver
        backend = bk.get_backend(cfg.baseband_format_type)
        n_endpoints = len(cfg.udp_receiver_address)
        my = shard_streams(n_endpoints, world, rank)
        if not my:
            print(f"rank {rank}: no UDP endpoints assigned")
            return 0
        bits = abs(cfg.baseband_input_bits)
        block_bytes = cfg.baseband_input_count * bits // 8 * \
            bk.get_data_stream_count(cfg.baseband_format_type)
        pipes = {ep: make(cfg, reserved) for ep in my}
        q: "_queue.Queue" = _queue.Queue(maxsize=2 * len(my))
        state = {"n": 0, "stop": False}

        def stop():
            return state["stop"] or (max_blocks is not None and
                                     state["n"] >= max_blocks)

        def receiver(ep):
            assembler = BlockAssembler(backend, block_bytes)
            provider = UdpPacketProvider(cfg.udp_receiver_address[ep],
                                         cfg.udp_receiver_port[ep])
            try:
                run_receiver(provider, assembler,
                             lambda blk, ts: q.put((ep, blk, ts)), stop)
            finally:
                provider.close()

        # fold position of a UDP block: from its begin counter where the
        # packet format carries one, else from the block ordinal
        payload = backend.packet_payload_size - backend.packet_header_size
        per_packet = (payload * 8 // bits // n_streams
                      if backend.packet_header_size else 0)
        fold_first: dict = {}
        fold_seen: dict = {}
        fold_warned: set = set()

        def udp_fold_position(ep, ts):
            k = fold_seen.get(ep, 0)
            fold_seen[ep] = k + 1
            if not per_packet:
                return k * cfg.baseband_input_count
            first = fold_first.setdefault(ep, ts)
            n0 = (ts - first) * per_packet
            if n0 != k * cfg.baseband_input_count and ep not in fold_warned:
                fold_warned.add(ep)
                print(f"[srtb_amd] fold: endpoint {ep} dropped data before "
                      f"block {ts}; the phase follows the packet counter")
            return n0

        # a block whose begin counter does not follow its predecessor's (for
        # formats that carry one): data was dropped in between
        incoh_last: dict = {}

        def udp_dropped(ep, ts):
            last = incoh_last.get(ep)
            incoh_last[ep] = ts
            if not per_packet or last is None:
                return False
            return (ts - last) * per_packet != cfg.baseband_input_count

        threads = [threading.Thread(target=receiver, args=(ep,), daemon=True)
                   for ep in my]
        for t in threads:
            t.start()
        while not stop():
            try:
                ep, blk, ts = q.get(timeout=0.2)
            except _queue.Empty:
                continue
            if fold_on:
                n0 = udp_fold_position(ep, ts)
                pipes[ep].fold_position(n0)
            for products in process(pipes[ep], blk, ts):
                writer.push(products)
            fil_append(pipes[ep], ep, len(my))
            if incoh_on:
                incoh_block_done(pipes[ep], ep, len(my),
                                 dropped=udp_dropped(ep, ts))
            if fold_on:
                fold_block_done(pipes[ep], n0, ep, len(my))
            state["n"] += 1
            gui_update(pipes[ep], state["n"], len(writer.written))
        state["stop"] = True
        n_blocks = state["n"]

    if write_all_f is not None:
        write_all_f.close()
    for ws in fil_writers.values():
        for w in ws:
            w.close()
    for out in incoh_outs.values():
        out.close()
    for ep, out in fold_outs.items():
        out.flush(pipe if cfg.input_file_path else pipes[ep])
    elapsed = time.time() - t0
    if gui is not None:
        # keep serving the last frames briefly (the reference GUI keeps its
        # windows open after the pipeline drains)
        if gui_linger > 0:
            time.sleep(gui_linger)
        gui.stop()
    writer.close()  # flush the async write pool before the summary
    stats = agg.reduce()
    if rank == 0:
        sps = stats.blocks * cfg.baseband_input_count / max(elapsed, 1e-9)
        print(f"[srtb_amd] blocks={stats.blocks} detections={stats.detections} "
              f"signal_counts={stats.signal_counts} "
              f"zapped_channels={stats.zapped_channels} "
              f"written={len(writer.written)} "
              f"throughput={sps / 1e6:.1f} Msamples/s "
              f"real_time_ratio={sps / cfg.baseband_sample_rate:.2f}")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
