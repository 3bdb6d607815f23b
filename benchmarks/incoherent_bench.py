#!/usr/bin/env python3
"""What the incoherent DM-offset search costs, at the J1644-4559 shape.

One engine built like bench.py's (2^30 2-bit samples per block, DM -478.8 with
its overlap rounded for tscrunch) with the filterbank plane on (tscrunch 16,
32-bit), and one IncoherentSearch of --trials offsets spanning +-span pc cm^-3
on its [R][C] plane.  --channels is the engine's spectrum_channel_count;
fscrunch 1 makes it the plane's C as well (4096 by default).

  --mode wall (default)
     Runs of --blocks blocks alternate between the engine alone and the engine
     with the search attached (fed after every submit, two blocks in flight,
     as srtb-backend does), --repeats times each; a run is timed by the host
     clock around work that ends in a synchronise.  Reports ms per block per
     run, the medians and their difference, and the two kernels event-timed on
     the last plane.
  --mode kernels
     Only --blocks search blocks on a fixed plane and nothing else, for a
     profiler run of its own:
       rocprofv3 --kernel-trace --stats -d prof_out -- \\
           python benchmarks/incoherent_bench.py --mode kernels
     (k_incoh_dedisperse, k_incoh_combine and k_incoh_detect run once per
     block each).
  --mode search
     The searcher alone: runs of --blocks blocks of submit_plane on a fixed
     plane (two in flight), --repeats of them, each timed by the host clock
     around work that ends in the last wait.  With --normalize the runs
     alternate between a searcher without the per-channel normalisation and
     one with it (--normalize-blocks), in the same process; it reports ms per
     block per run, the medians, the spread (max - min) of the repeats and
     the on - off cost with its share of the off block time.

Prints one JSON line.
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
    ap.add_argument("--mode", choices=("wall", "kernels", "search"),
                    default="wall")
    ap.add_argument("--normalize", action="store_true",
                    help="--mode search: alternate normalisation off and on")
    ap.add_argument("--normalize-blocks", type=int, default=8)
    ap.add_argument("--n", type=int, default=2**30)
    ap.add_argument("--channels", type=int, default=2**12)
    ap.add_argument("--blocks", type=int, default=24)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--tscrunch", type=int, default=16)
    ap.add_argument("--trials", type=int, default=256)
    ap.add_argument("--span", type=float, default=0.5)
    ap.add_argument("--max-boxcar", type=int, default=256)
    ap.add_argument("--kernel-iters", type=int, default=20)
    return ap.parse_args(argv)


def main(argv=None):
    args = parse_args(argv)
    import torch
    from srtb_amd import ref
    from srtb_amd.ops import native

    assert torch.cuda.is_available(), "incoherent_bench.py requires a GPU"
    torch.cuda.set_device(0)
    C = native()

    n, s = args.n, args.channels
    freq_low, bandwidth, sample_rate, dm = 1437.0, -64.0, 128e6, -478.80
    reserved = ref.nsamps_reserved(n, s, freq_low, bandwidth, sample_rate, dm,
                                   True, time_multiple=args.tscrunch)
    hdr = ref.filterbank_header_fields(freq_low, bandwidth, sample_rate, s,
                                       args.tscrunch, 1)
    rows = (n - reserved) // (2 * s * args.tscrunch)
    offsets = np.linspace(-args.span, args.span, args.trials).tolist()
    search_kw = dict(
        rows=rows, channels=hdr["nchans"], fch1=hdr["fch1"], foff=hdr["foff"],
        tsamp=hdr["tsamp"], offsets=offsets, snr_threshold=8.0,
        max_boxcar=args.max_boxcar)
    search = C.IncoherentSearch(**search_kw)
    shape = {"n": n, "channels": s, "nsamps_reserved": reserved,
             "tscrunch": args.tscrunch, "rows": rows,
             "out_channels": hdr["nchans"], "trials": args.trials,
             "span": args.span, "d_max": search.d_max,
             "max_boxcar": args.max_boxcar}
    rng = np.random.default_rng(1234)

    if args.mode == "kernels":
        plane = torch.from_numpy(rng.chisquare(
            32, (rows, hdr["nchans"])).astype(np.float32)).cuda()
        pending = []
        for _ in range(args.blocks):
            pending.append(search.submit_plane(plane))
            if len(pending) >= 2:
                search.wait(pending.pop(0))
        for k in pending:
            search.wait(k)
        torch.cuda.synchronize()
        print(json.dumps({"shape": shape, "mode": "kernels",
                          "blocks": args.blocks}), flush=True)
        return

    if args.mode == "search":
        plane = torch.from_numpy(rng.chisquare(
            32, (rows, hdr["nchans"])).astype(np.float32)).cuda()
        searchers = {"off": search}
        if args.normalize:
            searchers["on"] = C.IncoherentSearch(
                normalize=True, normalize_blocks=args.normalize_blocks,
                **search_kw)

        def run_search(s, blocks):
            pending = []
            for _ in range(blocks):
                pending.append(s.submit_plane(plane))
                if len(pending) >= 2:
                    s.wait(pending.pop(0))
            for k in pending:
                s.wait(k)

        for s_ in searchers.values():  # warm-up
            run_search(s_, 4)
        ms = {name: [] for name in searchers}
        for _ in range(args.repeats):
            for name, s_ in searchers.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                run_search(s_, args.blocks)
                ms[name].append(
                    (time.perf_counter() - t0) / args.blocks * 1e3)
        out = {"shape": shape, "mode": "search",
               "blocks_per_run": args.blocks}
        for name, v in ms.items():
            out[f"ms_per_block_{name}"] = [round(x, 4) for x in v]
            out[f"median_{name}_ms"] = round(statistics.median(v), 4)
            out[f"spread_{name}_ms"] = round(max(v) - min(v), 4)
        if args.normalize:
            extra = out["median_on_ms"] - out["median_off_ms"]
            out["normalize_blocks"] = args.normalize_blocks
            out["normalize_extra_ms_per_block"] = round(extra, 4)
            out["normalize_share_of_off"] = round(
                extra / out["median_off_ms"], 4)
            out["plane_bytes"] = rows * hdr["nchans"] * 4
        print(json.dumps(out), flush=True)
        return

    nc = n // 2
    lo = round((1422.0 - freq_low) / bandwidth * (nc - 1))
    hi = round((1418.0 - freq_low) / bandwidth * (nc - 1))
    eng = C.PipelineEngine(
        n=n, nbits=2, channels=s, freq_low=freq_low, bandwidth=bandwidth,
        sample_rate=sample_rate, dm=dm, rfi_threshold=1.5,
        sk_threshold=1.05, snr_threshold=8.0, max_boxcar=256,
        nsamps_reserved=reserved, zap_ranges=[[int(lo), int(hi)]],
        use_phase_table=False, enable_rfi_s1=True, enable_sk=True,
        n_slots=2, fft_backend=0, fil_tscrunch=args.tscrunch, fil_fscrunch=1,
        fil_nbits=32)
    assert (eng.filterbank_rows, eng.filterbank_channels) == \
        (rows, hdr["nchans"])
    pinned = [torch.from_numpy(rng.integers(
        0, 256, eng.raw_bytes, dtype=np.uint8)).pin_memory()
        for _ in range(2)]

    def run(blocks, with_search):
        inflight = []

        def drain():
            slot, k = inflight.pop(0)
            eng.wait(slot)
            if k is not None:
                search.wait(k)
            return slot

        last = None
        for i in range(blocks):
            slot = eng.submit(pinned[i % 2])
            k = search.submit(eng, slot) if with_search else None
            inflight.append((slot, k))
            if len(inflight) >= 2:
                last = drain()
        while inflight:
            last = drain()
        eng.synchronize()
        return last

    run(4, False)  # warm-up
    run(4, True)
    ms = {"off": [], "on": []}
    for _ in range(args.repeats):
        for name in ("off", "on"):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            run(args.blocks, name == "on")
            ms[name].append((time.perf_counter() - t0) / args.blocks * 1e3)

    # ---- the two kernels alone, on the last block's plane ----
    slot = run(2, False)
    plane = eng.filterbank_power(slot)
    d_max = search.d_max
    window = torch.cat([torch.zeros(d_max, hdr["nchans"], device="cuda"),
                        plane]).contiguous()
    delays = search.delays().cuda()

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

    # the binding also reduces the table (min, max) and allocates: an upper
    # bound of the kernel, the profiler run has the kernel alone
    dedisp_ms = event_ms(lambda: C.incoh_dedisperse(window, delays, rows))
    Y = C.incoh_dedisperse(window, delays, rows)
    detect_ms = event_ms(lambda: C.incoh_detect(Y, 8.0, args.max_boxcar))
    gathers = args.trials * rows * hdr["nchans"]

    med = {k: statistics.median(v) for k, v in ms.items()}
    print(json.dumps({
        "shape": shape, "mode": "wall", "blocks_per_run": args.blocks,
        "ms_per_block_off": [round(x, 3) for x in ms["off"]],
        "ms_per_block_on": [round(x, 3) for x in ms["on"]],
        "median_off_ms": round(med["off"], 3),
        "median_on_ms": round(med["on"], 3),
        "extra_ms_per_block": round(med["on"] - med["off"], 3),
        "dedisperse_call_ms": round(dedisp_ms, 4),
        "dedisperse_Ggathers_per_s": round(gathers / dedisp_ms / 1e6, 1),
        "detect_call_ms": round(detect_ms, 4),
        "per_offset_us": round((dedisp_ms + detect_ms) / args.trials * 1e3, 2),
    }), flush=True)


if __name__ == "__main__":
    main()
