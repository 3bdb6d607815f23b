"""GPU-side orchestration helpers above the native engine.

- DualPolPipeline: one packet stream fanning out to 2 polarization sample
  streams (naocpsr_snap1 / gznupsr_a1 / byte-interleaved cpsr2), each run
  through the full chain (reference unpack_pipe.hpp:146-390 fan-out).
- DmTrialSweep: coherent DM-trial search over one block (Crab giant-pulse
  search config of BASELINE.json) using the engine's per-submit DM override:
  one whole chain per trial.
- DmTrialSearch: the same search from ONE forward spectrum per block (engine
  submit_trials): only the backward half runs per trial, and the per-trial
  peak S/N, boxcar width and arrival sample are found on the GPU.
"""

from __future__ import annotations

from dataclasses import dataclass

import numpy as np

from .. import ref
from ..config import Config


def filterbank_engine_kwargs(cfg: Config) -> dict:
    """Engine keywords that switch the per-stream filterbank plane on ({}
    while neither ``filterbank_output_path`` nor ``incoherent_dm_offsets`` is
    set, and with ``filterbank_polarization``, where a PolCombiner makes the
    one plane)."""
    plane = cfg.filterbank_output_path or cfg.incoherent_dm_offsets.strip()
    if not plane or cfg.filterbank_polarization:
        return {}
    return {"fil_tscrunch": cfg.filterbank_tscrunch,
            "fil_fscrunch": cfg.filterbank_fscrunch,
            "fil_nbits": cfg.filterbank_nbits}


def fold_engine_kwargs(cfg: Config) -> dict:
    """Engine keywords that switch pulsar folding on ({} while
    ``fold_output_path`` is unset)."""
    if not cfg.fold_output_path:
        return {}
    f0, f1 = cfg.fold_spin()
    return {"fold_nbin": cfg.fold_nbin, "fold_f0": f0, "fold_f1": f1,
            "fold_phase0": cfg.fold_phase_offset}


def _make_engine(C, cfg: Config, nsamps_reserved: int, nbits: int,
                 n: int | None = None, n_slots: int = 2,
                 max_dm_trials: int = 0, **engine_kwargs):
    nc = (n or cfg.baseband_input_count) // 2
    ranges = ref.parse_rfi_freq_list(cfg.mitigate_rfi_freq_list)
    bins = ref.rfi_ranges_to_bins(cfg.baseband_freq_low,
                                  cfg.baseband_bandwidth, nc, ranges)
    return C.PipelineEngine(
        n=n or cfg.baseband_input_count, nbits=nbits,
        channels=cfg.spectrum_channel_count, freq_low=cfg.baseband_freq_low,
        bandwidth=cfg.baseband_bandwidth, sample_rate=cfg.baseband_sample_rate,
        dm=cfg.dm, rfi_threshold=cfg.mitigate_rfi_average_method_threshold,
        sk_threshold=cfg.mitigate_rfi_spectral_kurtosis_threshold,
        snr_threshold=cfg.signal_detect_signal_noise_threshold,
        max_boxcar=cfg.signal_detect_max_boxcar_length,
        nsamps_reserved=nsamps_reserved,
        zap_ranges=[[int(a), int(b)] for a, b in bins],
        use_phase_table=False, enable_rfi_s1=True, enable_sk=True,
        n_slots=n_slots, max_dm_trials=max_dm_trials, **engine_kwargs)


class DualPolPipeline:
    """Process a 2-polarization packed stream: one unpack fan-out on the GPU,
    then the per-pol chain through one engine per polarization."""

    def __init__(self, cfg: Config, nsamps_reserved: int, kind: str):
        import torch
        from ..ops import native
        self.torch = torch
        self.C = native()
        self.kind = kind  # "interleave" | "naocpsr_snap1" | "gznupsr_a1"
        self.cfg = cfg
        # per-pol blocks have baseband_input_count samples each
        self.engines = [
            _make_engine(self.C, cfg, nsamps_reserved, nbits=-8),
            _make_engine(self.C, cfg, nsamps_reserved, nbits=-8),
        ]

    def submit_block(self, raw: np.ndarray) -> dict:
        """Fan one packed block out and enqueue both polarization chains;
        returns a handle for wait_block.  The handle owns the fan-out
        tensors: they must stay alive until the engines drained them (the
        caching allocator would otherwise recycle their memory under the
        engine streams)."""
        torch = self.torch
        n = self.cfg.baseband_input_count
        raw_t = torch.from_numpy(np.ascontiguousarray(raw)).cuda()
        if self.kind == "gznupsr_a1":
            pols = self.C.unpack_gznupsr_a1(raw_t, 2)
        else:
            pols = self.C.unpack_2pol(raw_t, self.kind)
        slots = []
        for eng, pol in zip(self.engines, pols):
            assert pol.numel() == n
            slots.append(eng.submit_samples(pol))
        return {"slots": slots, "pols": pols, "raw": raw_t}

    def wait_block(self, handle: dict) -> list[dict]:
        out = []
        for eng, slot in zip(self.engines, handle["slots"]):
            res = eng.wait(slot)
            res["slot"] = slot
            out.append(res)
        return out

    def process_block(self, raw: np.ndarray) -> list[dict]:
        """raw: packed bytes holding 2 * baseband_input_count int8 samples.
        Returns one result dict per polarization."""
        return self.wait_block(self.submit_block(raw))


@dataclass
class DmTrial:
    dm: float
    counts: list
    zero_count: int
    peak_snr: float


class DmTrialSweep:
    """Coherent DM-trial sweep over one baseband block.

    The block is uploaded once; each trial then re-runs the WHOLE chain
    (unpack, forward FFT, r2c finish, mean power, and the backward half) with
    a different dedispersion DM (on-the-fly phase) — nothing is reused between
    trials.  DmTrialSearch shares the forward half.  The best trial is the one
    with the highest peak SNR in its time series.
    """

    def __init__(self, cfg: Config, nsamps_reserved: int = 0):
        import torch
        from ..ops import native
        self.torch = torch
        self.C = native()
        self.cfg = cfg
        self.eng = _make_engine(self.C, cfg, nsamps_reserved,
                                nbits=cfg.baseband_input_bits)

    def sweep(self, raw: np.ndarray, dms: list[float]) -> list[DmTrial]:
        torch = self.torch
        raw_t = torch.from_numpy(np.ascontiguousarray(raw)).cuda()
        trials = []
        # keep both engine slots in flight: trial i+1 uploads/computes while
        # trial i drains (the serial submit→wait loop left the GPU idle
        # during each host-side readback)
        inflight: list[tuple[float, int]] = []
        n_slots = self.eng.n_slots

        def drain_one():
            dm, slot = inflight.pop(0)
            res = self.eng.wait(slot)
            ts = self.eng.time_series(slot)
            std = float(ts.std())
            peak = float(ts.max()) / std if std > 0 else 0.0
            trials.append(DmTrial(dm=float(dm), counts=res["counts"],
                                  zero_count=res["zero_count"],
                                  peak_snr=peak))

        for dm in dms:
            inflight.append((float(dm),
                             self.eng.submit(raw_t, dm_override=float(dm))))
            if len(inflight) >= n_slots:
                drain_one()
        while inflight:
            drain_one()
        return trials

    def best(self, trials: list[DmTrial]) -> DmTrial:
        return max(trials, key=lambda t: t.peak_snr)


@dataclass
class DmTrialResult:
    dm: float
    counts: list
    zero_count: int
    peak_snr: float    # highest peak S/N over the raw series and the ladder
    peak_boxcar: int   # boxcar length attaining it (1 = raw series)
    peak_index: int    # its sample index (boxcar indexing)


class DmTrialSearch:
    """Coherent DM-trial search from one forward spectrum per block.

    The engine runs the forward half of the chain once per block and keeps
    the spectrum on the device; every trial DM runs only the backward half
    (RFI + dedispersion, waterfall transform, detection) from it.  Peaks come
    from the GPU, in units of the rms the detection threshold uses, so no
    per-trial host pass over the series is needed.  Both engine slots are
    used: block i+1 uploads while block i runs its trials.
    """

    def __init__(self, cfg: Config, dms: list[float],
                 nsamps_reserved: int = 0):
        import torch
        from ..ops import native
        self.torch = torch
        self.C = native()
        self.cfg = cfg
        self.dms = [float(d) for d in dms]
        if not self.dms:
            raise ValueError("DmTrialSearch needs at least one trial DM")
        self.eng = _make_engine(self.C, cfg, nsamps_reserved,
                                nbits=cfg.baseband_input_bits,
                                max_dm_trials=len(self.dms))

    def submit(self, raw) -> dict:
        """Enqueue one block's trials; raw is a numpy array or a (host or
        device) tensor of the block's bytes.  The handle keeps the block
        alive until wait()."""
        torch = self.torch
        if not isinstance(raw, torch.Tensor):
            raw = torch.from_numpy(np.ascontiguousarray(raw))
        return {"slot": self.eng.submit_trials(raw, self.dms), "raw": raw}

    def wait(self, handle: dict) -> list[DmTrialResult]:
        out = []
        for t in self.eng.wait_trials(handle["slot"]):
            p = max(t["peaks"], key=lambda q: q["snr"])
            out.append(DmTrialResult(
                dm=float(t["dm"]), counts=t["counts"],
                zero_count=t["zero_count"], peak_snr=float(p["snr"]),
                peak_boxcar=int(p["boxcar_length"]),
                peak_index=int(p["index"])))
        return out

    def search(self, raw) -> list[DmTrialResult]:
        return self.wait(self.submit(raw))

    def best(self, results: list[DmTrialResult]) -> DmTrialResult:
        return max(results, key=lambda t: t.peak_snr)
