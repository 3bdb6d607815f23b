#!/usr/bin/env python3
"""What the continuous filterbank output costs, at the J1644-4559 shape.

One process, two engines built like bench.py's (2^30 2-bit samples per block,
2048 channels, DM -478.8 with its overlap rounded for tscrunch): one with the
feature off, one with it on (tscrunch 16, fscrunch 1, 8-bit by default).

  1. Block time.  Runs of --blocks blocks alternate between the two engines,
     --repeats times each; a run is timed by the host clock around work that
     ends in an engine synchronise.  Reports ms per block per run, the medians
     and their difference.
  2. Detect kernel alone.  filterbank_detect on the slot's [2048][2^18]
     waterfall (4.3 GB, far larger than the caches), warm, event-timed, next to
     the time-series kernels, which read the same bytes.  Reports ms and bytes
     read per second for both.

Prints one JSON line.  Usage:
  python benchmarks/filterbank_bench.py [--blocks 24] [--repeats 3]
                                        [--tscrunch 16] [--fscrunch 1]
                                        [--nbits 8] [--n 1073741824]
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
    ap.add_argument("--tscrunch", type=int, default=16)
    ap.add_argument("--fscrunch", type=int, default=1)
    ap.add_argument("--nbits", type=int, default=8)
    ap.add_argument("--kernel-iters", type=int, default=20)
    return ap.parse_args(argv)


def main(argv=None):
    args = parse_args(argv)
    import torch
    from srtb_amd import ref
    from srtb_amd.ops import native

    assert torch.cuda.is_available(), "filterbank_bench.py requires a GPU"
    torch.cuda.set_device(0)
    C = native()

    n, s = args.n, args.channels
    freq_low, bandwidth, sample_rate, dm = 1437.0, -64.0, 128e6, -478.80
    nc = n // 2
    lo = round((1422.0 - freq_low) / bandwidth * (nc - 1))
    hi = round((1418.0 - freq_low) / bandwidth * (nc - 1))
    # both engines get the overlap the feature needs, so they do equal work
    reserved = ref.nsamps_reserved(n, s, freq_low, bandwidth, sample_rate, dm,
                                   True, time_multiple=args.tscrunch)

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
        "on": engine(fil_tscrunch=args.tscrunch, fil_fscrunch=args.fscrunch,
                     fil_nbits=args.nbits),
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

    # ---- the detect kernel alone, on the last block's waterfall ----
    eng = engines["on"]
    slot = run(eng, 2)
    wf = eng.waterfall(slot)
    valid = eng.filterbank_rows * args.tscrunch
    ts_count = eng.ts_count

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

    detect_ms = event_ms(lambda: C.filterbank_detect(
        wf, None, valid, args.tscrunch, args.fscrunch, bandwidth > 0))
    series_ms = event_ms(lambda: C.time_series(wf, None, ts_count))
    detect_bytes = s * valid * 8
    series_bytes = s * ts_count * 8

    med = {k: statistics.median(v) for k, v in ms.items()}
    print(json.dumps({
        "shape": {"n": n, "channels": s, "waterfall_len": eng.waterfall_len,
                  "nsamps_reserved": reserved, "tscrunch": args.tscrunch,
                  "fscrunch": args.fscrunch, "nbits": args.nbits,
                  "rows": eng.filterbank_rows,
                  "out_channels": eng.filterbank_channels},
        "blocks_per_run": args.blocks,
        "ms_per_block_off": [round(x, 3) for x in ms["off"]],
        "ms_per_block_on": [round(x, 3) for x in ms["on"]],
        "median_off_ms": round(med["off"], 3),
        "median_on_ms": round(med["on"], 3),
        "extra_ms_per_block": round(med["on"] - med["off"], 3),
        "detect_kernel_ms": round(detect_ms, 4),
        "detect_read_GBps": round(detect_bytes / detect_ms / 1e6, 1),
        "time_series_ms": round(series_ms, 4),
        "time_series_read_GBps": round(series_bytes / series_ms / 1e6, 1),
    }), flush=True)


if __name__ == "__main__":
    main()
