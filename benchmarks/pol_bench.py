#!/usr/bin/env python3
"""What the polarization products cost, at the J1644-4559 per-pol shape.

One process, no children; --timeout (seconds) ends it by SIGALRM.

  1. Kernel alone.  Two [2048][2^18] complex waterfalls (4.3 GB each, far
     larger than the caches), warm, --kernel-iters event-timed launches per
     measurement, --repeats rounds alternating between
       pair: two back-to-back filterbank_detect launches, one per waterfall,
       I:    one filterbank_detect_pol launch, state I,
       IQUV: one filterbank_detect_pol launch, state IQUV.
     All three read the same bytes, so the pair's time is the one to match.
  2. Block time of a dual-polarization pipeline (two engines fed unpacked
     samples that already sit on the device, both slots in flight), --repeats
     runs of --blocks blocks alternating between
       per_stream_8bit: each engine makes its own 8-bit plane (no combiner),
       iquv_f32:        plain engines + PolCombiner, IQUV, float32,
       i_8bit:          plain engines + PolCombiner, I, 8-bit.

Prints one JSON line.  Usage:
  python benchmarks/pol_bench.py [--blocks 12] [--repeats 3] [--n 268435456]
                                 [--kernel-len 262144] [--skip-blocks]
"""

import argparse
import json
import os
import signal
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def parse_args(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=2**28,
                    help="samples per polarization per block (block time)")
    ap.add_argument("--channels", type=int, default=2**11)
    ap.add_argument("--kernel-len", type=int, default=2**18,
                    help="waterfall length of the kernel-alone measurement")
    ap.add_argument("--blocks", type=int, default=12)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--tscrunch", type=int, default=16)
    ap.add_argument("--fscrunch", type=int, default=1)
    ap.add_argument("--kernel-iters", type=int, default=20)
    ap.add_argument("--skip-blocks", action="store_true")
    ap.add_argument("--timeout", type=int, default=540)
    return ap.parse_args(argv)


def kernel_alone(C, torch, ref, args):
    s, length = args.channels, args.kernel_len
    t, f = args.tscrunch, args.fscrunch
    gen = torch.Generator(device="cuda").manual_seed(7)
    wfs = [torch.view_as_complex(torch.randn(
        s, length, 2, device="cuda", generator=gen)) for _ in range(2)]

    def pair():
        C.filterbank_detect(wfs[0], None, length, t, f, False)
        C.filterbank_detect(wfs[1], None, length, t, f, False)

    def pol(state):
        return lambda: C.filterbank_detect_pol(
            wfs[0], wfs[1], None, None, length, t, f, False,
            ref.POL_STATES[state])

    cases = {"pair": pair, "I": pol("I"), "IQUV": pol("IQUV")}

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

    ms = {k: [] for k in cases}
    for _ in range(args.repeats):
        for name, fn in cases.items():
            ms[name].append(event_ms(fn))
    read_bytes = 2 * s * length * 8
    out = {"shape": [s, length], "tscrunch": t, "fscrunch": f,
           "launches_per_measurement": args.kernel_iters,
           "read_bytes": read_bytes}
    for name, v in ms.items():
        med = statistics.median(v)
        out[name + "_ms"] = [round(x, 4) for x in v]
        out[name + "_median_ms"] = round(med, 4)
        out[name + "_read_GBps"] = round(read_bytes / med / 1e6, 1)
    del wfs
    torch.cuda.empty_cache()
    return out


def block_time(C, torch, ref, args):
    n, s, t, f = args.n, args.channels, args.tscrunch, args.fscrunch
    freq_low, bandwidth, sample_rate, dm = 1437.0, -64.0, 128e6, -478.80
    nc = n // 2
    lo = round((1422.0 - freq_low) / bandwidth * (nc - 1))
    hi = round((1418.0 - freq_low) / bandwidth * (nc - 1))
    reserved = ref.nsamps_reserved(n, s, freq_low, bandwidth, sample_rate, dm,
                                   True, time_multiple=t)

    def engine(**kw):
        return C.PipelineEngine(
            n=n, nbits=-8, channels=s, freq_low=freq_low, bandwidth=bandwidth,
            sample_rate=sample_rate, dm=dm, rfi_threshold=1.5,
            sk_threshold=1.05, snr_threshold=8.0, max_boxcar=256,
            nsamps_reserved=reserved, zap_ranges=[[int(lo), int(hi)]],
            use_phase_table=False, enable_rfi_s1=True, enable_sk=True,
            n_slots=2, fft_backend=0, **kw)

    def combiner(state, nbits):
        return C.PolCombiner(
            n=n, channels=s, nsamps_reserved=reserved, tscrunch=t, fscrunch=f,
            reverse=bandwidth > 0, pol_state=ref.POL_STATES[state],
            nbits=nbits)

    fil = dict(fil_tscrunch=t, fil_fscrunch=f, fil_nbits=8)
    configs = {
        "per_stream_8bit": ([engine(**fil), engine(**fil)], None),
        "iquv_f32": ([engine(), engine()], combiner("IQUV", 32)),
        "i_8bit": ([engine(), engine()], combiner("I", 8)),
    }
    gen = torch.Generator(device="cuda").manual_seed(11)
    pols = [torch.randn(n, device="cuda", generator=gen).mul_(16).round_()
            for _ in range(2)]

    def run(engines, comb, blocks):
        inflight = []

        def drain():
            slots, k = inflight.pop(0)
            for e, sl in zip(engines, slots):
                e.wait(sl)
            if comb is not None:
                comb.wait(k)

        for _ in range(blocks):
            slots = [e.submit_samples(p) for e, p in zip(engines, pols)]
            k = None
            if comb is not None:
                k = comb.submit(engines[0], slots[0], engines[1], slots[1])
            inflight.append((slots, k))
            if len(inflight) >= 2:
                drain()
        while inflight:
            drain()
        for e in engines:
            e.synchronize()

    for engines, comb in configs.values():  # warm-up
        run(engines, comb, 4)
    ms = {k: [] for k in configs}
    for _ in range(args.repeats):
        for name, (engines, comb) in configs.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            run(engines, comb, args.blocks)
            ms[name].append((time.perf_counter() - t0) / args.blocks * 1e3)
    out = {"n_per_pol": n, "channels": s, "nsamps_reserved": reserved,
           "tscrunch": t, "fscrunch": f, "blocks_per_run": args.blocks}
    for name, v in ms.items():
        out[name + "_ms_per_block"] = [round(x, 3) for x in v]
        out[name + "_median_ms"] = round(statistics.median(v), 3)
    return out


def main(argv=None):
    args = parse_args(argv)
    signal.alarm(args.timeout)
    import torch
    from srtb_amd import ref
    from srtb_amd.ops import native

    assert torch.cuda.is_available(), "pol_bench.py requires a GPU"
    torch.cuda.set_device(0)
    C = native()
    result = {"kernel": kernel_alone(C, torch, ref, args)}
    if not args.skip_blocks:
        result["block"] = block_time(C, torch, ref, args)
    print(json.dumps(result), flush=True)


if __name__ == "__main__":
    main()
