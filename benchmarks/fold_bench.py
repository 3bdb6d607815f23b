#!/usr/bin/env python3
"""What online pulsar folding costs, at the J1644-4559 shape.

One process, two engines built like bench.py's (2^30 2-bit samples per block,
2048 channels, DM -478.8): one with the feature off, one folding into 1024
bins at P = 0.455 s.

  1. Block time.  Runs of --blocks blocks alternate between the two engines,
     --repeats times each; a run is timed by the host clock around work that
     ends in an engine synchronise.  Reports ms per block per run, the medians
     and their difference.
  2. Fold kernels alone.  fold_block (turn table + counts + accumulate) on the
     slot's [2048][2^18] waterfall (4.3 GB, far larger than the caches), warm,
     event-timed, next to filterbank_detect at tscrunch 16 on the same tensor
     in the same process: that kernel reads the same bytes, so it is the
     yardstick.  The module-level fold_block also uploads its two phase words
     per call, which the engine does with an async copy; that is inside the
     timed span.

Prints one JSON line.  Usage:
  python benchmarks/fold_bench.py [--blocks 24] [--repeats 3] [--nbin 1024]
                                  [--period 0.455] [--n 1073741824]
"""

import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def parse_args(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=2**30)
    ap.add_argument("--channels", type=int, default=2**11)
    ap.add_argument("--blocks", type=int, default=24)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--nbin", type=int, default=1024)
    ap.add_argument("--period", type=float, default=0.455)
    ap.add_argument("--tscrunch", type=int, default=16)
    ap.add_argument("--kernel-iters", type=int, default=20)
    return ap.parse_args(argv)


def main(argv=None):
    args = parse_args(argv)
    import torch
    from srtb_amd import ref
    from srtb_amd.ops import native

    assert torch.cuda.is_available(), "fold_bench.py requires a GPU"
    torch.cuda.set_device(0)
    C = native()

    n, s = args.n, args.channels
    freq_low, bandwidth, sample_rate, dm = 1437.0, -64.0, 128e6, -478.80
    nc = n // 2
    lo = round((1422.0 - freq_low) / bandwidth * (nc - 1))
    hi = round((1418.0 - freq_low) / bandwidth * (nc - 1))
    # the overlap rounded for the yardstick's tscrunch, for both engines
    reserved = ref.nsamps_reserved(n, s, freq_low, bandwidth, sample_rate, dm,
                                   True, time_multiple=args.tscrunch)
    f0 = 1.0 / args.period

    def engine(**kw):
        return C.PipelineEngine(
            n=n, nbits=2, channels=s, freq_low=freq_low, bandwidth=bandwidth,
            sample_rate=sample_rate, dm=dm, rfi_threshold=1.5,
            sk_threshold=1.05, snr_threshold=8.0, max_boxcar=256,
            nsamps_reserved=reserved, zap_ranges=[[int(lo), int(hi)]],
            use_phase_table=False, enable_rfi_s1=True, enable_sk=True,
            n_slots=2, fft_backend=0, **kw)

    engines = {
        "off": engine(),
        "on": engine(fold_nbin=args.nbin, fold_f0=f0, fold_f1=0.0,
                     fold_phase0=0.0),
    }
    rng = np.random.default_rng(1234)
    pinned = [torch.from_numpy(rng.integers(
        0, 256, engines["off"].raw_bytes, dtype=np.uint8)).pin_memory()
        for _ in range(2)]

    def run(eng, blocks):
        inflight = []
        last = None
        for i in range(blocks):
            inflight.append(eng.submit(pinned[i % 2]))
            if len(inflight) >= 2:
                last = inflight.pop(0)
                eng.wait(last)
        while inflight:
            last = inflight.pop(0)
            eng.wait(last)
        eng.synchronize()
        return last

    for eng in engines.values():  # warm-up
        run(eng, 4)
    ms = {"off": [], "on": []}
    for _ in range(args.repeats):
        for name in ("off", "on"):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            run(engines[name], args.blocks)
            ms[name].append((time.perf_counter() - t0) / args.blocks * 1e3)

    # ---- the fold kernels alone, on the last block's waterfall ----
    eng = engines["on"]
    slot = run(eng, 2)
    _n0, phi, dphi = eng.fold_words(slot)
    wf = eng.waterfall(slot)
    valid = (n - reserved) // (2 * s)
    acc = torch.zeros(s, args.nbin, dtype=torch.float64, device="cuda")
    hits = torch.zeros(args.nbin, dtype=torch.int64, device="cuda")
    weights = torch.zeros(s, dtype=torch.int64, device="cuda")

    def event_ms(fn):
        fn()
        fn()  # warm
        torch.cuda.synchronize()
        e0 = torch.cuda.Event(enable_timing=True)
        e1 = torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(args.kernel_iters):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / args.kernel_iters

    fold_ms = event_ms(lambda: C.fold_block(
        wf, None, valid, args.nbin, phi, dphi, acc, hits, weights))
    detect_ms = event_ms(lambda: C.filterbank_detect(
        wf, None, valid, args.tscrunch, 1, bandwidth > 0))
    nbytes = s * valid * 8

    med = {k: statistics.median(v) for k, v in ms.items()}
    print(json.dumps({
        "shape": {"n": n, "channels": s, "waterfall_len": eng.waterfall_len,
                  "nsamps_reserved": reserved, "valid_columns": valid,
                  "nbin": args.nbin, "period": args.period,
                  "turns_per_block": valid * dphi / 2.0 ** 64},
        "blocks_per_run": args.blocks,
        "ms_per_block_off": [round(x, 3) for x in ms["off"]],
        "ms_per_block_on": [round(x, 3) for x in ms["on"]],
        "median_off_ms": round(med["off"], 3),
        "median_on_ms": round(med["on"], 3),
        "extra_ms_per_block": round(med["on"] - med["off"], 3),
        "fold_kernels_ms": round(fold_ms, 4),
        "fold_read_GBps": round(nbytes / fold_ms / 1e6, 1),
        "detect_kernel_ms": round(detect_ms, 4),
        "detect_read_GBps": round(nbytes / detect_ms / 1e6, 1),
        "fold_over_detect": round(fold_ms / detect_ms, 3),
    }), flush=True)


if __name__ == "__main__":
    main()
