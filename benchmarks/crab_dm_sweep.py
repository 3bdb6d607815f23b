#!/usr/bin/env python3
"""BASELINE.json config 5: Crab giant-pulse search — 16-bit baseband,
coherent DM-trial sweep + boxcar detection, DM trials sharded across GPUs.

Two modes over this rank's share of the DM trial list:

  --mode resubmit (default)  DmTrialSweep: the block is uploaded once and
      every trial re-runs the WHOLE chain through the engine's per-submit DM
      override (unpack, forward FFT, r2c finish and mean power included);
      the peak S/N is ts.max()/ts.std() on the host side.
  --mode shared              DmTrialSearch: one forward half per block, one
      backward half per trial from the retained spectrum; peak S/N, boxcar
      width and sample come from the GPU peak kernel.

Per-trial peak SNRs are all-gathered and rank 0 reports the best trial.

Usage: python benchmarks/crab_dm_sweep.py [--n 2**28] [--trials 16]
                                          [--mode resubmit|shared]
       torchrun --nproc-per-node 8 benchmarks/crab_dm_sweep.py
The band, sample rate and bit width default to the Crab configuration and can
be set for other geometries (--bits 2 --freq-low 1437 --bandwidth -64 ...).
"""

import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def parse_args(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=2**28)
    ap.add_argument("--channels", type=int, default=2**11)
    ap.add_argument("--trials", type=int, default=16)
    ap.add_argument("--dm-center", type=float, default=56.77)  # Crab DM
    ap.add_argument("--dm-span", type=float, default=8.0)
    ap.add_argument("--inject", action="store_true",
                    help="inject a dispersed pulse at dm-center")
    ap.add_argument("--mode", choices=("resubmit", "shared"),
                    default="resubmit")
    ap.add_argument("--bits", type=int, default=-16)
    ap.add_argument("--freq-low", type=float, default=1000.0)
    ap.add_argument("--bandwidth", type=float, default=500.0)
    ap.add_argument("--sample-rate", type=float, default=1e9)
    return ap.parse_args(argv)


def make_config(args):
    from srtb_amd.config import Config
    cfg = Config()
    cfg.baseband_input_count = args.n
    cfg.spectrum_channel_count = args.channels
    cfg.baseband_input_bits = args.bits
    cfg.baseband_freq_low = args.freq_low
    cfg.baseband_bandwidth = args.bandwidth
    cfg.baseband_sample_rate = args.sample_rate
    cfg.dm = args.dm_center
    cfg.mitigate_rfi_average_method_threshold = 1e30
    cfg.mitigate_rfi_spectral_kurtosis_threshold = 1e30
    cfg.signal_detect_signal_noise_threshold = 8.0
    cfg.signal_detect_max_boxcar_length = 256
    return cfg


def make_block(args, cfg):
    from srtb_amd.config import Config
    from srtb_amd.pipeline.cpu import synthesize_dispersed_pulse
    if args.inject:
        if args.bits != -16:
            raise SystemExit("--inject synthesizes 16-bit baseband only")
        cfg8 = Config()
        for k in ("baseband_input_count", "spectrum_channel_count",
                  "baseband_freq_low", "baseband_bandwidth",
                  "baseband_sample_rate", "dm"):
            setattr(cfg8, k, getattr(cfg, k))
        cfg8.baseband_input_bits = -8
        t = 0.4 * args.n / cfg.baseband_sample_rate
        raw8 = synthesize_dispersed_pulse(cfg8, t, pulse_amp=35.0,
                                          noise_sigma=2.0)
        return (raw8.view(np.int8).astype(np.int16) * 64).view(np.uint8)
    rng = np.random.default_rng(7)
    return rng.integers(0, 256, args.n * abs(args.bits) // 8, dtype=np.uint8)


def trial_dms(args):
    dms = np.linspace(args.dm_center - args.dm_span,
                      args.dm_center + args.dm_span, args.trials)
    if args.inject:
        dms[args.trials // 2] = args.dm_center  # ensure the true DM is a trial
    return dms


class ModeRunner:
    """One mode's engine plus its timed search over a block; returns
    [(dm, peak_snr)] per trial."""

    def __init__(self, mode, cfg, my_dms):
        from srtb_amd.pipeline.gpu import DmTrialSearch, DmTrialSweep
        self.mode = mode
        self.my_dms = my_dms
        if mode == "shared":
            self.search = DmTrialSearch(cfg, my_dms, nsamps_reserved=0)
        else:
            self.sweep = DmTrialSweep(cfg, nsamps_reserved=0)

    def warmup(self, raw):
        if self.mode == "shared":
            self.run(raw)
        else:
            self.sweep.sweep(raw, self.my_dms[:1])

    def run(self, raw):
        if self.mode == "shared":
            import torch
            # upload inside the timed region, as DmTrialSweep.sweep does
            raw_t = torch.from_numpy(np.ascontiguousarray(raw)).cuda()
            return [(r.dm, r.peak_snr) for r in self.search.search(raw_t)]
        return [(t.dm, t.peak_snr)
                for t in self.sweep.sweep(raw, self.my_dms)]


def main():
    args = parse_args()

    import torch

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    torch.cuda.set_device(local_rank)
    if world > 1:
        torch.distributed.init_process_group(backend="nccl")

    cfg = make_config(args)
    raw = make_block(args, cfg)
    dms = trial_dms(args)
    my_dms = [float(d) for i, d in enumerate(dms) if i % world == rank]

    runner = ModeRunner(args.mode, cfg, my_dms)
    runner.warmup(raw)
    if world > 1:
        torch.distributed.barrier()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    trials = runner.run(raw)
    torch.cuda.synchronize()
    if world > 1:
        torch.distributed.barrier()
    elapsed = time.perf_counter() - t0

    # gather (dm, peak_snr) across ranks
    local = torch.tensor(trials, dtype=torch.float64, device="cuda")
    if world > 1:
        sizes = [len(dms) // world + (1 if r < len(dms) % world else 0)
                 for r in range(world)]
        gathered = [torch.zeros(sz, 2, dtype=torch.float64, device="cuda")
                    for sz in sizes]
        torch.distributed.all_gather(gathered, local)
        allt = torch.cat(gathered, 0)
    else:
        allt = local
    if rank == 0:
        best = allt[allt[:, 1].argmax()]
        print(json.dumps({
            "metric": "DM trials/s (coherent, 16-bit baseband)",
            "value": round(len(dms) / elapsed, 2),
            "unit": "trials/s",
            "n_gpus": world,
            "trials": len(dms),
            "ms_per_trial": round(elapsed / max(len(my_dms), 1) * 1e3, 1),
            "samples_per_trial": args.n,
            "best_dm": round(float(best[0]), 3),
            "best_peak_snr": round(float(best[1]), 1),
            "higher_is_better": True,
            "scaling": "strong",
            "mode": args.mode,
        }), flush=True)
    if world > 1:
        torch.distributed.destroy_process_group()


if __name__ == "__main__":
    main()
