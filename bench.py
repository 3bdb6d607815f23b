#!/usr/bin/env python3
"""Flagship benchmark: the J1644-4559 single-pulse pipeline on MI355X.

One step = --blocks-per-step full baseband blocks (default 2^30 samples
each, 2-bit, the J1644-4559 observation config of BASELINE.json, with the
DM-478.8 dedispersion overlap of ~23.5 M samples reserved and reprocessed
per block as the reference does) through the native engine:

  H2D → unpack → R2C FFT (2^30) → RFI s1 + manual zap + coherent dedispersion
  (fused) → waterfall batched C2C (2048 ch) → spectral-kurtosis RFI →
  time-series + boxcar single-pulse detection → detection-counter readback,

with double-buffered slots (2 HIP streams/GPU).  Multi-GPU: one rank per GPU
(torch.distributed over RCCL/xGMI), each rank processing its own baseband
stream (weak scaling — the reference shards streams/polarizations/beams the
same way) and all-reducing the per-block detection counters.

Usage: python bench.py --gpus N --steps K --warmup W
                       [--dump-outputs DIR] [--full]
(For N>1 the driver launches via torch.distributed.run; RANK/LOCAL_RANK/
WORLD_SIZE/MASTER_* are read from the environment.)

A plain run sets up, warms up, times the K steps and prints ONE JSON line on
rank 0 with the whole-job Msamples/s.  --dump-outputs DIR additionally writes
what the last timed step computed (see dump_outputs) so two builds can be
compared output for output; the inputs are seeded and identical from run to
run.  --full is reserved for supplementary measurements that need runs of
their own; the flagship benchmark has none today, so it changes nothing yet.
"""

import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


# --dump-outputs keeps the waterfall whole up to this many bytes, else a
# fixed seeded sample of this size; with the sample's index array of the
# same size and the ~1 MB time series the whole dump stays under 64 MB
DUMP_WATERFALL_BYTES = 16 << 20
DUMP_SAMPLE_SEED = 20240


def dump_outputs(out_dir, eng, last_step):
    """Write the outputs of the last timed step as out_dir/<name>.npy.

    last_step: [(slot, result)] of the step's blocks in submission order.
      detect_counts.npy      float64 [blocks, 1 + n_boxcar]: zero_count, then
                             the detection count of every boxcar length
      detect_boxcars.npy     float64 [n_boxcar]: the boxcar lengths
      detect_thresholds.npy  float64 [blocks, n_thresholds]
      time_series.npy        float32 [ts_count]: last block, whole
      waterfall.npy          float32 [K, 2] (re, im): last block's dedispersed
                             waterfall, whole (row-major) if it fits
                             DUMP_WATERFALL_BYTES, else the elements listed in
      waterfall_index.npy    float64 [K]: flat indices of the seeded sample
    """
    import torch

    os.makedirs(out_dir, exist_ok=True)

    def save(name, a, dtype):
        np.save(os.path.join(out_dir, name + ".npy"),
                np.ascontiguousarray(a, dtype=dtype))

    save("detect_counts",
         [[r["zero_count"]] + [c for _, c in r["counts"]]
          for _, r in last_step], np.float64)
    save("detect_boxcars", [b for b, _ in last_step[-1][1]["counts"]],
         np.float64)
    save("detect_thresholds", [list(r["thresholds"]) for _, r in last_step],
         np.float64)

    # device buffers of the last block's slot are intact: nothing was
    # submitted after it and the engine is synchronized
    slot = last_step[-1][0]
    save("time_series", eng.time_series(slot).cpu().numpy(), np.float32)
    wf = torch.view_as_real(eng.waterfall(slot)).reshape(-1, 2)
    k = DUMP_WATERFALL_BYTES // 8
    if wf.shape[0] > k:
        idx = np.sort(np.random.default_rng(DUMP_SAMPLE_SEED).integers(
            0, wf.shape[0], k))
        save("waterfall_index", idx, np.float64)
        wf = wf[torch.from_numpy(idx).to(wf.device)]
    save("waterfall", wf.cpu().numpy(), np.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=8)
    ap.add_argument("--warmup", type=int, default=3)
    # NOTE: under torchrun pass --input-count, not --n: torchrun's argparse
    # greedily matches --n as an ambiguous prefix of its own --nnodes/... even
    # after the script positional.
    ap.add_argument("--n", "--input-count", dest="n", type=int, default=2**30,
                    help="baseband_input_count per block (J1644: 2^30)")
    ap.add_argument("--channels", type=int, default=2**11)
    ap.add_argument("--bits", type=int, default=2)
    ap.add_argument("--blocks-per-step", type=int, default=8,
                    help="baseband blocks processed per timed step (one "
                    "block ~20 ms; >1 keeps the timed region long enough "
                    "for external GPU-utilization sampling)")
    ap.add_argument("--no-reserve", action="store_true",
                    help="disable the dedispersion overlap reservation "
                    "(nsamps_reserved=0; NOT the honest J1644 config)")
    ap.add_argument("--phase-table", action="store_true",
                    help="cache dedispersion phase factors (fixed DM); "
                    "default recomputes fp64 phase per block like the reference")
    ap.add_argument("--no-rfi", action="store_true")
    ap.add_argument("--fft", choices=["native", "hipfft", "auto"],
                    default="native",
                    help="FFT backend (hand-written Stockham vs hipFFT)")
    ap.add_argument("--graph", action="store_true",
                    help="capture the per-block chain into hipGraphs")
    ap.add_argument("--slots", type=int, default=2,
                    help="double-buffered engine slots (streams); 2 measured "
                    "fastest (r02 A/B: 17.4/18.7/20.5/17.8 ms per block at "
                    "2/3/4/6 slots — deeper concurrency degrades aggregate "
                    "HBM efficiency)")
    ap.add_argument("--backend", choices=["nccl", "gloo"], default="nccl",
                    help="torch.distributed backend for world>1 (nccl=RCCL "
                    "over xGMI, one rank per GPU; gloo validates the "
                    "distributed path with several ranks sharing one GPU)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps write the last step's "
                    "outputs (detection counters, time series, waterfall "
                    "sample) as DIR/<name>.npy")
    ap.add_argument("--full", action="store_true",
                    help="also run supplementary measurements beyond the "
                    "headline figure (none exist yet; a plain run is "
                    "already lean)")
    args = ap.parse_args()

    import torch

    world_size = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    n_gpus = world_size if world_size > 1 else args.gpus
    distributed = world_size > 1

    assert torch.cuda.is_available(), "bench.py requires a GPU"
    torch.cuda.set_device(local_rank % torch.cuda.device_count())

    if distributed:
        torch.distributed.init_process_group(backend=args.backend)
    # collective tensors live on the GPU for RCCL, on the host for gloo
    coll_dev = "cuda" if args.backend == "nccl" else "cpu"

    from srtb_amd.ops import native
    from srtb_amd import ref
    C = native()

    # J1644-4559 observation config (reference userspace/srtb_config_1644-4559.cfg)
    n = args.n
    s = args.channels
    freq_low = 1437.0     # 1405 + 64/2
    bandwidth = -64.0
    sample_rate = 128e6
    dm = -478.80
    rfi_threshold = 1.5
    sk_threshold = 1.05
    snr = 8.0
    max_boxcar = 256
    nc = n // 2
    # manual zap 1418-1422 MHz → bin range (negative bandwidth)
    lo = round((1422.0 - freq_low) / bandwidth * (nc - 1))
    hi = round((1418.0 - freq_low) / bandwidth * (nc - 1))
    zap_ranges = [[int(lo), int(hi)]]

    # dedispersion overlap: adjacent blocks share `reserved` samples which
    # are reprocessed next block (reference coherent_dedispersion.hpp:87-128);
    # at DM 478.8 on this band that is ~23.5 M of 2^30 (~2.2%).  Throughput
    # below counts only the (n - reserved) NEW samples per block.
    reserved = 0 if args.no_reserve else ref.nsamps_reserved(
        n, s, freq_low, bandwidth, sample_rate, dm, True)

    eng = C.PipelineEngine(
        n=n, nbits=args.bits, channels=s, freq_low=freq_low,
        bandwidth=bandwidth, sample_rate=sample_rate, dm=dm,
        rfi_threshold=rfi_threshold, sk_threshold=sk_threshold,
        snr_threshold=snr, max_boxcar=max_boxcar, nsamps_reserved=reserved,
        zap_ranges=zap_ranges, use_phase_table=args.phase_table,
        enable_rfi_s1=not args.no_rfi, enable_sk=True, n_slots=args.slots,
        fft_backend={"native": 0, "hipfft": 1, "auto": 2}[args.fft],
        use_hip_graph=args.graph)

    # synthetic 2-bit baseband noise, pinned, one buffer per slot
    rng = np.random.default_rng(1234 + rank)
    raw_bytes = eng.raw_bytes
    pinned = []
    for _ in range(max(args.slots, 2)):
        t = torch.from_numpy(rng.integers(0, 256, raw_bytes, dtype=np.uint8))
        pinned.append(t.pin_memory())

    # Detection-stat aggregation over RCCL: per-block counters go out as
    # ASYNC all-reduces (async_op=True — RCCL runs them on its own stream,
    # overlapped with the next blocks' compute); handles are only waited
    # when their rotating buffer is reused and at drain.  Nothing blocking
    # sits on the submit path.
    n_cbuf = max(args.slots, 2)
    counts_dev = [torch.zeros(4, dtype=torch.int64, device=coll_dev)
                  for _ in range(n_cbuf)]
    pending_handles = [None] * n_cbuf
    agg_i = 0

    def agg(res):
        nonlocal agg_i
        b = agg_i % n_cbuf
        agg_i += 1
        if pending_handles[b] is not None:
            pending_handles[b].wait()
            pending_handles[b] = None
        c = [res["zero_count"]] + [cnt for _, cnt in res["counts"][:3]]
        counts_dev[b].copy_(torch.tensor(c, dtype=torch.int64))
        if distributed:
            pending_handles[b] = torch.distributed.all_reduce(
                counts_dev[b], async_op=True)

    def drain_handles():
        for b in range(n_cbuf):
            if pending_handles[b] is not None:
                pending_handles[b].wait()
                pending_handles[b] = None

    # (slot, result) of every block of the current run_steps call, in
    # submission order — what a caller of the engine receives per block
    results = []

    def run_steps(k):
        # keep ALL slots in flight (submit-ahead depth = n_slots); waiting
        # with only one block queued leaves the GPU idle during the host-side
        # stat aggregation (~20% measured on the J1644 config)
        results.clear()
        inflight = []

        def collect():
            slot = inflight.pop(0)
            res = eng.wait(slot)
            agg(res)
            results.append((slot, res))

        for i in range(k * args.blocks_per_step):
            inflight.append(eng.submit(pinned[i % len(pinned)]))
            if len(inflight) >= args.slots:
                collect()
        while inflight:
            collect()
        drain_handles()
        eng.synchronize()

    # warmup
    run_steps(args.warmup)

    if distributed:
        torch.distributed.barrier()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    run_steps(args.steps)
    torch.cuda.synchronize()
    if distributed:
        torch.distributed.barrier()
    t1 = time.perf_counter()

    elapsed = t1 - t0
    # max over ranks
    if distributed:
        e = torch.tensor([elapsed], dtype=torch.float64, device=coll_dev)
        torch.distributed.all_reduce(e, op=torch.distributed.ReduceOp.MAX)
        elapsed = float(e.item())

    # valid (new-sky) samples only: the overlap tail is reprocessed work
    n_valid = n - reserved
    blocks = args.steps * args.blocks_per_step
    samples_total = float(n_valid) * blocks * n_gpus
    msamps = samples_total / elapsed / 1e6
    ms_per_step = elapsed / args.steps * 1e3
    per_gpu_sps = float(n_valid) * blocks / elapsed
    real_time_ratio = per_gpu_sps / sample_rate

    if rank == 0:
        out = {
            "metric": "baseband Msamples/sec/node + real-time ratio, "
                      "J1644-4559 config at 1/2/4/8 MI355X",
            "value": round(msamps, 1),
            "unit": "Msamples/s",
            "n_gpus": n_gpus,
            "steps": args.steps,
            "warmup": args.warmup,
            "ms_per_step": round(ms_per_step, 3),
            "higher_is_better": True,
            "scaling": "weak",
            # BASELINE.md implied number: >= 1000 Msamples/s per stream
            # (real-time at the 1 Gsps production config) on A40-class hardware
            "vs_baseline": round(msamps / 1000.0, 2),
            "dtype": "fp32",
            "data": "synthetic",
            "config": {
                "model": "J1644-4559 coherent-dedispersion single-pulse pipeline",
                "baseband_input_count": n,
                "nsamps_reserved": reserved,
                "blocks_per_step": args.blocks_per_step,
                "baseband_input_bits": args.bits,
                "spectrum_channel_count": s,
                "dm": dm,
                "freq_low_MHz": freq_low,
                "bandwidth_MHz": bandwidth,
                "sample_rate": sample_rate,
                "rfi": (not args.no_rfi),
                "phase_table": bool(args.phase_table),
                "fft_backend": args.fft,
                "real_time_ratio_per_gpu": round(real_time_ratio, 1),
                "parallelism": f"stream-sharded dp{n_gpus}",
                "global_batch": n_gpus,
                "seq_len": n,
            },
        }
        print(json.dumps(out), flush=True)

    if args.dump_outputs and rank == 0:
        dump_outputs(args.dump_outputs, eng, results[-args.blocks_per_step:])

    if distributed:
        torch.distributed.destroy_process_group()


if __name__ == "__main__":
    main()
