#include "engine.h"

#include <roctracer/roctx.h>

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <stdexcept>
#include <string>

namespace srtb_hip {

namespace {
constexpr double kD = 4.148808e3;  // dispersion constant (MHz^2 pc^-1 cm^3 s)

// x turns, 0 <= x <= 1, as a wrapping 64-bit phase word (2^64 = one turn),
// rounded to nearest; 1.0 wraps to 0.  From 2^53 on the scaled value is an
// integer already, so only the range llrint can hold goes through it.
uint64_t fold_turns_to_word(double x) {
  const double v = std::ldexp(x, 64);
  if (v >= 0x1p64) return 0;
  if (v >= 0x1p63) return (uint64_t)v;
  return (uint64_t)std::llrint(v);
}

// rocTX ranges per pipeline stage (SRTB_ROCTX=1): the rocprofv3 marker
// domain shows unpack/fft/rfi/sk/detect spans per block — the reference's
// per-pipe thread names, in profiler form (SURVEY §5 tracing).
struct RoctxRange {
  bool on;
  explicit RoctxRange(const char* name)
      : on([] {
          static const bool enabled = [] {
            const char* e = std::getenv("SRTB_ROCTX");
            return e && std::atoi(e) != 0;
          }();
          return enabled;
        }()) {
    if (on) roctxRangePush(name);
  }
  ~RoctxRange() {
    if (on) roctxRangePop();
  }
};
}

PipelineEngine::PipelineEngine(const EngineConfig& cfg, int n_slots)
    : cfg_(cfg), n_slots_(n_slots) {
  n_ = cfg.baseband_input_count;
  nc_ = n_ / 2;
  s_ = cfg.spectrum_channel_count;
  if (s_ > nc_) s_ = nc_;  // reference watfft clamps (fft_pipe.hpp:300-306)
  l_ = nc_ / s_;
  const size_t reserved_bins = cfg.nsamps_reserved / s_;
  ts_count_ = (l_ > reserved_bins) ? l_ - reserved_bins : l_;

  const int bits = std::abs(cfg.baseband_input_bits);
  raw_bytes_ = n_ * (size_t)bits / 8;

  // boxcar ladder: 2, 4, ..., while <= max && < ts_count (the fused
  // ladder kernel handles up to 12 lengths = max boxcar 4096; exotic
  // configs beyond that are clamped rather than rejected)
  for (size_t L = 2;
       L <= cfg.max_boxcar_length && L < ts_count_ &&
       boxcar_lengths_.size() < 12;
       L *= 2)
    boxcar_lengths_.push_back(L);
  n_boxcars_ = (int)boxcar_lengths_.size();

  // SK corrected thresholds (reference rfi_mitigation.hpp:292-307)
  {
    const double M = (double)l_;
    double hi = cfg.sk_threshold, lo = 2.0 - hi;
    if (lo > hi) std::swap(lo, hi);
    const double corr = (M - 1.0) / (M + 1.0);
    sk_lo_ = (float)(lo * corr + 1.0);
    sk_hi_ = (float)(hi * corr + 1.0);
  }
  // normalization coefficient (reference rfi_mitigation_pipe.hpp:60-66)
  norm_coeff_ = (float)std::pow((double)nc_ * (double)nc_ / (double)s_, -0.5);

  f_min_ = cfg.freq_low;
  f_c_ = cfg.freq_low + cfg.bandwidth;
  df_ = cfg.bandwidth / (double)nc_;

  if (cfg.max_dm_trials < 0 || cfg.max_dm_trials > kMaxDmTrials)
    throw std::runtime_error("max_dm_trials must be in [0, " +
                             std::to_string(kMaxDmTrials) + "]");

  if (const size_t t = cfg.fil_tscrunch) {
    const size_t f = cfg.fil_fscrunch;
    auto pow2 = [](size_t x) { return x && !(x & (x - 1)); };
    if (!pow2(t) || t > kFilterbankMaxTscrunch)
      throw std::runtime_error(
          "filterbank: fil_tscrunch must be a power of two <= " +
          std::to_string(kFilterbankMaxTscrunch));
    if (!pow2(f) || s_ % f != 0)
      throw std::runtime_error(
          "filterbank: fil_fscrunch must be a power of two dividing the "
          "channel count");
    if (cfg.fil_nbits != 8 && cfg.fil_nbits != 32)
      throw std::runtime_error("filterbank: fil_nbits must be 8 or 32");
    if (cfg.max_dm_trials > 0)
      throw std::runtime_error(
          "filterbank: not together with max_dm_trials > 0 (a filterbank "
          "holds one DM per file)");
    if (l_ % 2 != 0)
      throw std::runtime_error(
          "filterbank: needs at least 2 time samples per channel");
    if (cfg.nsamps_reserved >= n_ ||
        (n_ - cfg.nsamps_reserved) % (2 * s_ * t) != 0)
      throw std::runtime_error(
          "filterbank: baseband_input_count - nsamps_reserved must be a "
          "positive multiple of 2 * channels * fil_tscrunch = " +
          std::to_string(2 * s_ * t));
    fil_v_ = (n_ - cfg.nsamps_reserved) / (2 * s_);
    fil_r_ = fil_v_ / t;
    fil_c_ = s_ / f;
  }

  if (cfg.fold_nbin) {
    if (cfg.fold_nbin < kFoldMinBins || cfg.fold_nbin > kFoldMaxBins)
      throw std::runtime_error("fold: fold_nbin must be in " +
                               std::to_string(kFoldMinBins) + ".." +
                               std::to_string(kFoldMaxBins));
    if (!(cfg.fold_f0 > 0.0) || !std::isfinite(cfg.fold_f0))
      throw std::runtime_error("fold: fold_f0 must be positive");
    if (!(cfg.fold_f0 * (double)(2 * s_) / cfg.sample_rate < 1.0))
      throw std::runtime_error(
          "fold: fold_f0 is too high, one waterfall sample (2 * channels / "
          "sample_rate) must be shorter than a period");
    if (!std::isfinite(cfg.fold_f1))
      throw std::runtime_error("fold: fold_f1 must be finite");
    if (!std::isfinite(cfg.fold_phase0))
      throw std::runtime_error("fold: fold_phase0 must be finite");
    if (cfg.max_dm_trials > 0)
      throw std::runtime_error(
          "fold: fold_nbin > 0 not together with max_dm_trials > 0 (a "
          "profile holds one DM)");
    if (cfg.nsamps_reserved >= n_ ||
        (n_ - cfg.nsamps_reserved) % (2 * s_) != 0)
      throw std::runtime_error(
          "fold: baseband_input_count - nsamps_reserved must be a positive "
          "multiple of 2 * channels = " + std::to_string(2 * s_) +
          " (nsamps_reserved)");
    fold_v_ = (n_ - cfg.nsamps_reserved) / (2 * s_);
    fold_step_ = fold_turns_to_word(cfg.fold_f0 / cfg.sample_rate);
  }

  const int np = reduce_partials();
  for (int i = 0; i < n_slots_; ++i) slots_.emplace_back(new Slot());
  for (auto& sp : slots_) {
    Slot& s = *sp;
    check_hip(hipStreamCreateWithFlags(&s.stream, hipStreamNonBlocking),
              "stream create");
    check_hip(hipEventCreateWithFlags(&s.done, hipEventDisableTiming),
              "event create");
    check_hip(hipMalloc(&s.raw, raw_bytes_), "raw alloc");
    check_hip(hipMalloc(&s.samples, n_ * sizeof(float)), "samples alloc");
    check_hip(hipMalloc(&s.spec, (nc_ + 1) * sizeof(float2)), "spec alloc");
    check_hip(hipMalloc(&s.s2s4, s_ * sizeof(float2)), "s2s4 alloc");
    check_hip(hipMalloc(&s.flags, s_), "flags alloc");
    check_hip(hipMalloc(&s.ts, ts_count_ * sizeof(float)), "ts alloc");
    check_hip(hipMalloc(&s.ts_partial,
                        (size_t)time_series_chunks(ts_count_) * ts_count_ *
                            sizeof(float)),
              "ts partial alloc");
    check_hip(hipMalloc(&s.cumsum, ts_count_ * sizeof(float)), "cumsum alloc");
    check_hip(hipMalloc(&s.box, ts_count_ * sizeof(float)), "box alloc");
    check_hip(hipMalloc(&s.scan_scratch,
                        std::max(4096, scan_scratch_size(ts_count_)) *
                            sizeof(float)),
              "scan alloc");
    check_hip(hipMalloc(&s.partials, np * sizeof(double)), "partials alloc");
    if (n_boxcars_ > 0)
      check_hip(hipMalloc(&s.box_partials,
                          (size_t)n_boxcars_ * 2 * np * sizeof(double)),
                "box partials alloc");
    check_hip(hipMalloc(&s.mean_power, sizeof(double)), "mean alloc");
    check_hip(hipMalloc(&s.sums, 2 * sizeof(double)), "sums alloc");
    const int ncnt = 1 + 1 + n_boxcars_;  // zero_count + raw + boxcars
    check_hip(hipMalloc(&s.counters, ncnt * sizeof(unsigned)), "cnt alloc");
    check_hip(hipMalloc(&s.thresholds, (1 + n_boxcars_) * sizeof(float)),
              "thr alloc");
    check_hip(hipHostMalloc(&s.h_counters, ncnt * sizeof(unsigned)),
              "pinned cnt");
    check_hip(hipHostMalloc(&s.h_thresholds, (1 + n_boxcars_) * sizeof(float)),
              "pinned thr");
    s.last_row = plain_row(s);
    if (const size_t T = (size_t)cfg.max_dm_trials) {
      const size_t nthr = 1 + (size_t)n_boxcars_;
      check_hip(hipMalloc(&s.trial_w, nc_ * sizeof(float2)), "trial w alloc");
      check_hip(hipMalloc(&s.trial_plane, T * ts_count_ * sizeof(float)),
                "trial plane alloc");
      check_hip(hipMalloc(&s.trial_counters, T * ncnt * sizeof(unsigned)),
                "trial cnt alloc");
      check_hip(hipMalloc(&s.trial_thresholds, T * nthr * sizeof(float)),
                "trial thr alloc");
      check_hip(hipMalloc(&s.trial_peak_val, T * nthr * sizeof(float)),
                "trial peak alloc");
      check_hip(hipMalloc(&s.trial_peak_idx, T * nthr * sizeof(unsigned)),
                "trial peak idx alloc");
      check_hip(hipHostMalloc(&s.h_trial_counters, T * ncnt * sizeof(unsigned)),
                "pinned trial cnt");
      check_hip(hipHostMalloc(&s.h_trial_thresholds, T * nthr * sizeof(float)),
                "pinned trial thr");
      check_hip(hipHostMalloc(&s.h_trial_peak_val, T * nthr * sizeof(float)),
                "pinned trial peak");
      check_hip(hipHostMalloc(&s.h_trial_peak_idx, T * nthr * sizeof(unsigned)),
                "pinned trial peak idx");
      check_hip(hipMalloc(&s.peak_scratch, detect_peaks_scratch_bytes()),
                "peak scratch alloc");
    }
    if (fil_r_) {
      const size_t cells = fil_r_ * fil_c_;
      check_hip(hipMalloc(&s.fil_power, cells * sizeof(float)),
                "filterbank power alloc");
      if (cfg.fil_nbits == 8) {
        check_hip(hipMalloc(&s.fil_stats, 2 * fil_c_ * sizeof(float)),
                  "filterbank stats alloc");
        check_hip(hipMalloc(&s.fil_u8, cells), "filterbank u8 alloc");
        check_hip(hipMalloc(&s.fil_partials,
                            filterbank_stats_partials(fil_c_) * sizeof(double)),
                  "filterbank partials alloc");
        check_hip(hipHostMalloc(&s.h_fil_stats, 2 * fil_c_ * sizeof(float)),
                  "pinned filterbank stats");
        check_hip(hipHostMalloc(&s.h_fil, cells), "pinned filterbank");
      } else {
        check_hip(hipHostMalloc(&s.h_fil, cells * sizeof(float)),
                  "pinned filterbank");
      }
    }
    if (fold_v_) {
      const size_t nb = cfg.fold_nbin;
      check_hip(hipMalloc(&s.fold_acc, s_ * nb * sizeof(double)),
                "fold acc alloc");
      check_hip(hipMalloc(&s.fold_hits, nb * sizeof(uint64_t)),
                "fold hits alloc");
      check_hip(hipMalloc(&s.fold_weights, s_ * sizeof(uint64_t)),
                "fold weights alloc");
      check_hip(hipMalloc(&s.fold_dwords, 2 * sizeof(uint64_t)),
                "fold words alloc");
      check_hip(hipMalloc(&s.fold_table,
                          fold_table_words(fold_v_) * sizeof(uint32_t)),
                "fold table alloc");
      check_hip(hipHostMalloc(&s.h_fold_words, 2 * sizeof(uint64_t)),
                "pinned fold words");
      check_hip(hipMemset(s.fold_acc, 0, s_ * nb * sizeof(double)),
                "fold acc clear");
      check_hip(hipMemset(s.fold_hits, 0, nb * sizeof(uint64_t)),
                "fold hits clear");
      check_hip(hipMemset(s.fold_weights, 0, s_ * sizeof(uint64_t)),
                "fold weights clear");
      // the slot's stream does not order itself after the null stream
      check_hip(hipDeviceSynchronize(), "fold clear sync");
    }
    // backend selection (see EngineConfig::fft_backend): the forward
    // 2^29-class packed C2C always favors the native plan; the batched
    // backward favors rocFFT below the measured l_ = 2^17 crossover
    fused_unpack_off_ = std::getenv("SRTB_NO_FUSED_UNPACK") != nullptr;
    if (const char* sc = std::getenv("SRTB_SERIAL_CHAINS"))
      serial_chains_ = std::atoi(sc) != 0 ? 1 : 0;
    const int be = cfg.fft_backend;
    native_fft_ = (be == 0 || be == 2) && NativeFft::supported(nc_);
    native_bwd_ = native_fft_ && NativeFft::supported(l_) &&
                  (be == 0 || l_ >= (1ull << 17));
    fuse_r2c_ = false;
    if (native_fft_) {
      s.nfwd.plan(nc_, 1, -1, s.stream);
      // r2c pair-combine at the forward final pass's store (default where
      // the plan allows it, SRTB_FFT_R2C_FINAL=0 reverts): its mean-power
      // partials are one per workgroup, a count that comes from the plan
      if (const int rp = s.nfwd.r2c_final_partials())
        check_hip(hipMalloc(&s.r2c_final_partials, rp * sizeof(double)),
                  "r2c final partials alloc");
      if (native_bwd_) {
        // the RFI+dedispersion preop fuses into the backward's FIRST
        // pass; SRTB_FFT_BWD32=1 plans it 32-max-column + final-256 (the
        // pair32 kernel hid more of the per-bin fp64 phase at 6
        // waves/SIMD: kernel-sum favored pair32, 28.1 vs 28.7 ms/block,
        // wall favored the wide plan).  The column-polynomial phase
        // removes that VALU cost, see docs/fft_design.md.
        const char* b32 = std::getenv("SRTB_FFT_BWD32");
        if (b32 && std::atoi(b32) != 0)
          s.nbwd.plan(l_, s_, +1, s.stream, /*maxcol_log2=*/5,
                      /*final_log2=*/8);
        else
          s.nbwd.plan(l_, s_, +1, s.stream);
        // the fused SK sums are those of the transform's own output: with a
        // non-rectangular window the waterfall is de-applied afterwards, so
        // the sums come from sk_row_stats on the de-applied rows instead and
        // the partials do not exist (enqueue_back keys on the pointer)
        const int wpr = s.nbwd.dif_sk_wgs_per_row();
        if (cfg.enable_sk && wpr > 0 && cfg.window_kind == 0)
          check_hip(hipMalloc(&s.sk_dif_partials,
                              s_ * (size_t)wpr * sizeof(float2)),
                    "sk dif partials");
      } else {
        s.plans.create_c2c_only(l_, s_, s.stream);
      }
      check_hip(hipStreamSynchronize(s.stream), "fft table sync");
      // r2c-into-backward fusion (opt-in SRTB_FUSE_R2C=1): the
      // pair-combine runs at the backward first pass's load and the RFI
      // mean comes from Parseval on the packed spectrum — the standalone
      // 8.6 GB r2c pass disappears.  MEASURED SLOWER end-to-end (50.8 vs
      // 61.5 Gsps, r02): the combine adds a second 4.3 GB read + sincos
      // to the pass that was then the chain's critical kernel (per-bin
      // fp64 dedispersion), and the lost overlap outweighs the traffic
      // saved.  Not re-measured with the column-polynomial phase, which
      // this mode does not use (fft_col_preop_uses_poly).
      // Kept opt-in; numerics are exact (57 GPU tests pass either way).
      {
        const char* fe = std::getenv("SRTB_FUSE_R2C");
        const bool want = fe && std::atoi(fe) != 0;
        const int fwgs = s.nfwd.dif_sk_wgs_per_row();
        fuse_r2c_ = want && native_bwd_ && s.nbwd.first_pass_fusable() &&
                    fwgs > 0;
        if (fuse_r2c_) {
          fwd_pw_n_ = (size_t)fwgs;  // batch = 1
          check_hip(hipMalloc(&s.xbuf, nc_ * sizeof(float2)), "xbuf alloc");
          check_hip(hipMalloc(&s.fwd_pw, fwd_pw_n_ * sizeof(float2)),
                    "fwd pw alloc");
        }
      }
    } else {
      s.plans.create(n_, l_, s_, s.stream);
    }
  }

  if (cfg.window_kind != 0) {
    check_hip(hipMalloc(&window_, n_ * sizeof(float)), "window alloc");
    check_hip(build_window(window_, n_, cfg.window_kind, slots_[0]->stream),
              "window build");
    // K21: watfft window de-apply table of length l_ (reference
    // fft_pipe.hpp:350-358); only non-rectangle windows pay the pass
    check_hip(hipMalloc(&watfft_window_, l_ * sizeof(float)),
              "watfft window alloc");
    check_hip(build_window(watfft_window_, l_, cfg.window_kind,
                           slots_[0]->stream),
              "watfft window build");
    check_hip(hipStreamSynchronize(slots_[0]->stream), "window sync");
  }
  if (cfg.use_phase_table) {
    check_hip(hipMalloc(&phase_table_, nc_ * sizeof(float2)), "table alloc");
    check_hip(dedisp_phase_table(phase_table_, nc_, f_min_, f_c_, df_, cfg.dm,
                                 slots_[0]->stream),
              "phase table");
    check_hip(hipStreamSynchronize(slots_[0]->stream), "table sync");
  }
}

PipelineEngine::~PipelineEngine() {
  for (auto& sp : slots_) {
    if (sp->stream) (void)hipStreamSynchronize(sp->stream);
  }
  for (auto& sp : slots_) {
    Slot& s = *sp;
    s.plans.destroy();
    (void)hipFree(s.raw);
    (void)hipFree(s.samples);
    (void)hipFree(s.spec);
    (void)hipFree(s.s2s4);
    if (s.sk_dif_partials) (void)hipFree(s.sk_dif_partials);
    if (s.xbuf) (void)hipFree(s.xbuf);
    if (s.fwd_pw) (void)hipFree(s.fwd_pw);
    if (s.r2c_final_partials) (void)hipFree(s.r2c_final_partials);
    (void)hipFree(s.flags);
    (void)hipFree(s.ts);
    (void)hipFree(s.ts_partial);
    (void)hipFree(s.cumsum);
    (void)hipFree(s.box);
    (void)hipFree(s.scan_scratch);
    (void)hipFree(s.partials);
    if (s.box_partials) (void)hipFree(s.box_partials);
    (void)hipFree(s.mean_power);
    (void)hipFree(s.sums);
    (void)hipFree(s.counters);
    (void)hipFree(s.thresholds);
    (void)hipHostFree(s.h_counters);
    (void)hipHostFree(s.h_thresholds);
    if (s.trial_w) {
      (void)hipFree(s.trial_w);
      (void)hipFree(s.trial_plane);
      (void)hipFree(s.trial_counters);
      (void)hipFree(s.trial_thresholds);
      (void)hipFree(s.trial_peak_val);
      (void)hipFree(s.trial_peak_idx);
      (void)hipHostFree(s.h_trial_counters);
      (void)hipHostFree(s.h_trial_thresholds);
      (void)hipHostFree(s.h_trial_peak_val);
      (void)hipHostFree(s.h_trial_peak_idx);
      (void)hipFree(s.peak_scratch);
    }
    if (s.fil_power) {
      (void)hipFree(s.fil_power);
      if (s.fil_stats) (void)hipFree(s.fil_stats);
      if (s.fil_u8) (void)hipFree(s.fil_u8);
      if (s.fil_partials) (void)hipFree(s.fil_partials);
      if (s.h_fil_stats) (void)hipHostFree(s.h_fil_stats);
      (void)hipHostFree(s.h_fil);
    }
    if (s.fold_acc) {
      (void)hipFree(s.fold_acc);
      (void)hipFree(s.fold_hits);
      (void)hipFree(s.fold_weights);
      (void)hipFree(s.fold_dwords);
      (void)hipFree(s.fold_table);
      (void)hipHostFree(s.h_fold_words);
    }
    if (s.graph_exec) (void)hipGraphExecDestroy(s.graph_exec);
    if (s.done) (void)hipEventDestroy(s.done);
    if (s.stream) (void)hipStreamDestroy(s.stream);
  }
  if (phase_table_) (void)hipFree(phase_table_);
  if (window_) (void)hipFree(window_);
  if (watfft_window_) (void)hipFree(watfft_window_);
}

// The pre-op of the backward FFT's fused first pass (RFI s1 + manual zap +
// dedispersion at `dm`); meaningful only when that pass is fusable.
FftPreop PipelineEngine::make_preop(const Slot& s, double dm) const {
  FftPreop pre;
  if (native_bwd_ && s.nbwd.first_pass_fusable()) {
    pre.mean_power = cfg_.enable_rfi_s1 ? s.mean_power : nullptr;
    pre.threshold = cfg_.rfi_threshold;
    pre.norm_coeff = norm_coeff_;
    pre.n_zap = cfg_.n_zap_ranges;
    for (int i = 0; i < cfg_.n_zap_ranges; ++i) pre.zap[i] = cfg_.zap_ranges[i];
    pre.f_min = f_min_;
    pre.f_c = f_c_;
    pre.df = df_;
    pre.dm = dm;
    pre.table = phase_table_;
    pre.r2c_m = fuse_r2c_ ? nc_ : 0;
  }
  return pre;
}

PipelineEngine::ResultRow PipelineEngine::plain_row(Slot& s) const {
  return ResultRow{s.counters, s.thresholds, s.h_counters, s.h_thresholds};
}

PipelineEngine::ResultRow PipelineEngine::trial_row(Slot& s, int k) const {
  const size_t ncnt = 2 + (size_t)n_boxcars_, nthr = 1 + (size_t)n_boxcars_;
  return ResultRow{s.trial_counters + k * ncnt, s.trial_thresholds + k * nthr,
                   s.h_trial_counters + k * ncnt,
                   s.h_trial_thresholds + k * nthr};
}

// The per-block chain: the forward half (steps 1-3, independent of the DM)
// and the backward half (steps 4-11) in one go, in place on the slot's
// spectrum.  A DM-trial submission (enqueue_trials) runs the same two halves
// as one front and many backs.
void PipelineEngine::enqueue_chain(Slot& s, const uint8_t* dev_raw,
                                   const float* dev_samples, double dm,
                                   bool record_event) {
  if (std::isnan(dm)) dm = cfg_.dm;
  if (phase_table_ && dm != cfg_.dm)
    throw std::runtime_error("dm override requires use_phase_table=false");

  RoctxRange r_chain("srtb_block_chain");
  if (record_event) {
    const bool fuse_into_bwd = native_bwd_ && s.nbwd.first_pass_fusable();
    order_after_last_chain(
        s, fuse_into_bwd && serial_chains_ < 0 &&
               s.nbwd.preop_uses_poly(make_preop(s, dm)));
  }
  enqueue_front(s, dev_raw, dev_samples);
  enqueue_back(s, dm, plain_row(s), /*ts_dst=*/nullptr,
               /*keep_spectrum=*/false);
  if (fil_r_) enqueue_filterbank(s);
  if (fold_v_) enqueue_fold(s);
  s.trial_dms.clear();
  s.cur_trial = -1;
  if (record_event) {
    check_hip(hipEventRecord(s.done, s.stream), "event record");
    s.busy = true;
    last_chain_done_ = s.done;
  }
}

// Filterbank output of the block whose back half was just enqueued: one more
// read of the waterfall's first fil_v_ columns -> power plane -> (8-bit:
// channel statistics -> quantise) -> pinned host mirrors.  Reads the SK flags
// directly, so the waterfall stays un-zapped (see enqueue_back step 6).
void PipelineEngine::enqueue_filterbank(Slot& s) {
  hipStream_t st = s.stream;
  const size_t cells = fil_r_ * fil_c_;
  check_hip(filterbank_detect(s.wf, cfg_.enable_sk ? s.flags : nullptr, s_, l_,
                              fil_v_, cfg_.fil_tscrunch, cfg_.fil_fscrunch,
                              /*reverse=*/cfg_.bandwidth > 0, s.fil_power, st),
            "filterbank detect");
  if (cfg_.fil_nbits == 8) {
    float* mean = s.fil_stats;
    float* stddev = s.fil_stats + fil_c_;
    check_hip(filterbank_channel_stats(s.fil_power, fil_r_, fil_c_,
                                       s.fil_partials, mean, stddev, st),
              "filterbank stats");
    check_hip(filterbank_quantize(s.fil_power, mean, stddev, fil_r_, fil_c_,
                                  s.fil_u8, st),
              "filterbank quantize");
    check_hip(hipMemcpyAsync(s.h_fil, s.fil_u8, cells, hipMemcpyDeviceToHost,
                             st),
              "filterbank d2h");
    check_hip(hipMemcpyAsync(s.h_fil_stats, s.fil_stats,
                             2 * fil_c_ * sizeof(float), hipMemcpyDeviceToHost,
                             st),
              "filterbank stats d2h");
  } else {
    check_hip(hipMemcpyAsync(s.h_fil, s.fil_power, cells * sizeof(float),
                             hipMemcpyDeviceToHost, st),
              "filterbank d2h");
  }
}

// Phase words of the block about to be submitted to the (idle) slot, from the
// running stream position, which then advances by the block's new samples.
// Host side of docs/ARCHITECTURE.md "Pulsar folding": fp64 plus wrapping
// 64-bit integers; the integer product n0 * step keeps f0 * t exact over any
// observation length.
void PipelineEngine::stamp_fold(Slot& s) {
  const uint64_t n0 = fold_pos_;
  const uint64_t fresh = n_ - cfg_.nsamps_reserved;
  const double sr = cfg_.sample_rate, f1 = cfg_.fold_f1;
  const double t0 = (double)n0 / sr;
  const double t_mid = (double)(n0 + fresh / 2) / sr;
  const double p0 = cfg_.fold_phase0 - std::floor(cfg_.fold_phase0);
  const double v0 = std::ldexp(p0, 64);  // truncated, 2^64 wraps to 0
  const double q = 0.5 * f1 * t0 * t0;
  const uint64_t phi = (v0 >= 0x1p64 ? 0 : (uint64_t)v0) + n0 * fold_step_ +
                       fold_turns_to_word(q - std::floor(q));
  const uint64_t dphi =
      (uint64_t)(2 * s_) * fold_step_ +
      (uint64_t)(int64_t)std::llrint(
          std::ldexp(f1 * t_mid * ((double)(2 * s_) / sr), 64));
  s.fold_last = FoldWords{n0, phi, dphi};
  s.h_fold_words[0] = phi;
  s.h_fold_words[1] = dphi;
  fold_pos_ = n0 + fresh;
}

// Fold of the block whose back half was just enqueued: one more read of the
// waterfall's first fold_v_ columns.  The phase words travel from the slot's
// pinned pair to its device pair on the stream, so a captured chain replays
// with the words of the block it is launched for.  Reads the SK flags
// directly, like the filterbank.
void PipelineEngine::enqueue_fold(Slot& s) {
  check_hip(hipMemcpyAsync(s.fold_dwords, s.h_fold_words,
                           2 * sizeof(uint64_t), hipMemcpyHostToDevice,
                           s.stream),
            "fold words h2d");
  check_hip(fold_block(s.wf, cfg_.enable_sk ? s.flags : nullptr, s_, l_,
                       fold_v_, cfg_.fold_nbin, s.fold_dwords, s.fold_table,
                       s.fold_acc, s.fold_hits, s.fold_weights, s.stream),
            "fold");
}

PipelineEngine::FoldWords PipelineEngine::fold_words(int slot) const {
  if (!fold_v_) throw std::runtime_error("fold: fold_nbin = 0");
  return slots_.at(slot)->fold_last;
}

void PipelineEngine::fold_read(double* acc, uint64_t* hits,
                               uint64_t* weights) {
  if (!fold_v_) throw std::runtime_error("fold: fold_nbin = 0");
  synchronize();
  const size_t nb = cfg_.fold_nbin, cells = s_ * nb;
  std::vector<double> a(cells);
  std::vector<uint64_t> h(nb), w(s_);
  std::fill(acc, acc + cells, 0.0);
  std::fill(hits, hits + nb, 0);
  std::fill(weights, weights + s_, 0);
  for (auto& sp : slots_) {  // slot order: the sum is reproducible
    check_hip(hipMemcpy(a.data(), sp->fold_acc, cells * sizeof(double),
                        hipMemcpyDeviceToHost),
              "fold acc d2h");
    check_hip(hipMemcpy(h.data(), sp->fold_hits, nb * sizeof(uint64_t),
                        hipMemcpyDeviceToHost),
              "fold hits d2h");
    check_hip(hipMemcpy(w.data(), sp->fold_weights, s_ * sizeof(uint64_t),
                        hipMemcpyDeviceToHost),
              "fold weights d2h");
    for (size_t i = 0; i < cells; ++i) acc[i] += a[i];
    for (size_t i = 0; i < nb; ++i) hits[i] += h[i];
    for (size_t i = 0; i < s_; ++i) weights[i] += w[i];
  }
}

void PipelineEngine::fold_reset() {
  if (!fold_v_) throw std::runtime_error("fold: fold_nbin = 0");
  synchronize();
  const size_t nb = cfg_.fold_nbin;
  for (auto& sp : slots_) {
    check_hip(hipMemset(sp->fold_acc, 0, s_ * nb * sizeof(double)),
              "fold acc clear");
    check_hip(hipMemset(sp->fold_hits, 0, nb * sizeof(uint64_t)),
              "fold hits clear");
    check_hip(hipMemset(sp->fold_weights, 0, s_ * sizeof(uint64_t)),
              "fold weights clear");
  }
  check_hip(hipDeviceSynchronize(), "fold clear sync");
}

void PipelineEngine::order_after_last_chain(Slot& s, bool uses_poly) {
  // Slot scheduling.  With the per-bin fp64 dedispersion phase the fused
  // backward pass is VALU-bound and overlaps well with the other slot's
  // memory-bound passes, so the slots' chains run concurrently.  With the
  // column-polynomial phase every pass of the chain is memory-bound:
  // concurrent chains only share HBM (each pass takes twice as long), run in
  // lockstep and then issue their H2D copies together with the GPU idle
  // (measured: 20 % idle, 20.6 vs 16.9 ms per block).  So this chain's
  // kernels wait for the previously enqueued chain; the H2D copy enqueued
  // before it still overlaps that chain.  Not inside a graph capture.
  // A DM-trial submission is ordered as a whole: it waits when ANY of its
  // trials takes the polynomial path, and the next chain waits for its last
  // trial.  Whether that is the best rule for trial chains (many backward
  // halves per forward half) has not been measured.
  if (last_chain_done_ && last_chain_done_ != s.done &&
      (serial_chains_ > 0 || (serial_chains_ < 0 && uses_poly)))
    check_hip(hipStreamWaitEvent(s.stream, last_chain_done_, 0),
              "chain order");
}

// Forward half, steps 1-3: raw bytes (or samples) -> s.spec, the [Nc]
// forward spectrum, and the s.mean_power scalar.  Nothing here depends on
// the DM.
void PipelineEngine::enqueue_front(Slot& s, const uint8_t* dev_raw,
                                   const float* dev_samples) {
  hipStream_t st = s.stream;
  const bool fr2c = fuse_r2c_;  // r2c pair-combine fused into bwd load
  const float* fft_in = s.samples;
  // fused unpack: for the 2-bit rectangular-window native-forward case the
  // FFT's first column pass decodes the raw bytes itself (0.25 GB of byte
  // reads replace the unpack kernel's 4 GB write + the pass's 4 GB read)
  const int in_bits = cfg_.baseband_input_bits;
  const bool fuse_unpack = dev_raw && native_fft_ && !fused_unpack_off_ &&
                           (in_bits == 1 || in_bits == 2 || in_bits == 4 ||
                            in_bits == 8 || in_bits == -8 ||
                            in_bits == 16 || in_bits == -16) &&
                           !window_ && slots_[0]->nfwd.first_pass_fusable();
  if (dev_raw && !fuse_unpack) {
    // 1. unpack (+ window fused; default rectangle → none)
    check_hip(unpack(dev_raw, s.samples, n_, cfg_.baseband_input_bits,
                     window_, st),
              "unpack");
  } else if (!dev_raw && native_fft_) {
    // native fwd runs column passes in place on its input: copy the caller's
    // samples into the slot buffer first (D2D, overlapped on stream)
    check_hip(hipMemcpyAsync(s.samples, dev_samples, n_ * sizeof(float),
                             hipMemcpyDeviceToDevice, st),
              "samples d2d");
  } else if (!dev_raw) {
    fft_in = dev_samples;
  }
  if (native_fft_ && fr2c) {
    // 2. forward C2C of the packed-real view; the DIF store accumulates
    //    per-WG sum|Z|^2 and the RFI mean comes from Parseval — the
    //    standalone r2c pass (8.6 GB) is gone, its pair-combine runs at
    //    the backward first pass's load below.
    s.nfwd.exec(reinterpret_cast<float2*>(s.samples), s.spec, st,
                nullptr, cfg_.enable_rfi_s1 ? s.fwd_pw : nullptr,
                fuse_unpack ? dev_raw : nullptr, in_bits);
    if (cfg_.enable_rfi_s1)
      check_hip(r2c_mean_from_power(s.fwd_pw, fwd_pw_n_, s.spec, nc_,
                                    s.mean_power, st),
                "r2c mean");
  } else if (native_fft_ && s.r2c_final_partials) {
    // 2. forward transform of the packed-real view whose final pass combines
    //    the (k, Nc-k) pairs at its store: s.spec receives the r2c spectrum
    //    directly, with the FUSED mean-|X|^2, and the standalone r2c pass
    //    (8.6 GB) is gone
    NativeFft::R2cFinal rf;
    if (cfg_.enable_rfi_s1) {
      rf.mean_partials = s.r2c_final_partials;
      rf.out_mean = s.mean_power;
    }
    s.nfwd.exec(reinterpret_cast<float2*>(s.samples), s.spec, st, nullptr,
                nullptr, fuse_unpack ? dev_raw : nullptr, in_bits, nullptr,
                &rf);
  } else if (native_fft_) {
    // 2. forward C2C of the packed-real view + r2c post-process with FUSED
    //    mean-|X|^2 (saves the separate 4 GB mean_power pass)
    s.nfwd.exec(reinterpret_cast<float2*>(s.samples), s.spec, st,
                nullptr, nullptr, fuse_unpack ? dev_raw : nullptr, in_bits);
    check_hip(r2c_post_process(
                  s.spec, s.spec, nc_,
                  cfg_.enable_rfi_s1 ? s.partials : nullptr,
                  cfg_.enable_rfi_s1 ? s.mean_power : nullptr, st),
              "r2c post");
  } else {
    // 2. R2C forward (out-of-place; Nyquist bin written but ignored: the
    //    downstream count is Nc — reference drops it, fft_pipe.hpp:77)
    s.plans.exec_r2c(const_cast<float*>(fft_in), s.spec);
    // 3. mean |X|^2 over Nc
    if (cfg_.enable_rfi_s1)
      check_hip(mean_power(s.spec, nc_, s.partials, s.mean_power, st),
                "meanp");
  }
}

// Backward half, steps 4-11, at one DM: s.spec -> waterfall -> time series ->
// detection counters in `row`.  ts_dst (optional) receives a copy of the
// baseline-subtracted series; the series itself is always produced in s.ts,
// whose alignment the float4 reductions rely on (a row of the DM-time plane
// starts at k * ts_count floats, which need not be 16-byte aligned).
// keep_spectrum = false is the single-DM chain: s.spec is consumed in place.
// keep_spectrum = true leaves s.spec bit-for-bit intact and works in
// s.trial_w instead:
//   fused native backward   first column pass s.spec -> trial_w (the pre-op
//                           reads, never writes, its input), later passes in
//                           place in trial_w, final pass -> s.samples
//   everything else         out-of-place RFI+dedispersion s.spec -> trial_w,
//                           then the backward transform on trial_w (native:
//                           -> s.samples; rocFFT/hipFFT: in place, the
//                           waterfall is trial_w)
void PipelineEngine::enqueue_back(Slot& s, double dm, const ResultRow& row,
                                  float* ts_dst, bool keep_spectrum) {
  hipStream_t st = s.stream;
  const float2* table = phase_table_;
  const bool fr2c = fuse_r2c_;
  // RFI s1 + manual zap + dedispersion fuse into the backward FFT's first
  // column pass when the native planner allows it (step 4.+5. below)
  const bool fuse_into_bwd = native_bwd_ && s.nbwd.first_pass_fusable();
  const FftPreop pre = make_preop(s, dm);
  // 4.+5. RFI s1 + manual zap + dedispersion fused into the backward FFT's
  // first column pass when the native planner allows it (saves a full
  // read+write of the 4 GB spectrum); otherwise the standalone fused kernel.
  float2* wf;
  if (keep_spectrum && fuse_into_bwd) {
    s.nbwd.exec(s.spec, reinterpret_cast<float2*>(s.samples), st, &pre,
                s.sk_dif_partials, nullptr, 2, /*first_pass_out=*/s.trial_w);
    wf = reinterpret_cast<float2*>(s.samples);
  } else if (keep_spectrum) {
    check_hip(rfi_dedisperse_fused(
                  s.spec, s.trial_w, nc_,
                  cfg_.enable_rfi_s1 ? s.mean_power : nullptr,
                  cfg_.rfi_threshold, norm_coeff_, cfg_.zap_ranges,
                  cfg_.n_zap_ranges, f_min_, f_c_, df_, dm, table, st),
              "rfi+dedisp oop");
    if (native_bwd_) {
      s.nbwd.exec(s.trial_w, reinterpret_cast<float2*>(s.samples), st);
      wf = reinterpret_cast<float2*>(s.samples);
    } else {
      s.plans.exec_c2c_backward(s.trial_w);
      wf = s.trial_w;
    }
  } else if (fuse_into_bwd) {
    s.nbwd.exec(s.spec, reinterpret_cast<float2*>(s.samples), st, &pre,
                s.sk_dif_partials, nullptr, 2, fr2c ? s.xbuf : nullptr);
    wf = reinterpret_cast<float2*>(s.samples);
  } else {
    check_hip(rfi_dedisperse_fused(
                  s.spec, nc_, cfg_.enable_rfi_s1 ? s.mean_power : nullptr,
                  cfg_.rfi_threshold, norm_coeff_, cfg_.zap_ranges,
                  cfg_.n_zap_ranges, f_min_, f_c_, df_, dm, table, st),
              "rfi+dedisp");
    if (native_bwd_) {
      s.nbwd.exec(s.spec, reinterpret_cast<float2*>(s.samples), st);
      wf = reinterpret_cast<float2*>(s.samples);
    } else {
      s.plans.exec_c2c_backward(s.spec);
      wf = s.spec;
    }
  }
  s.wf = wf;
  if (watfft_window_)
    check_hip(window_deapply(wf, watfft_window_, s_ * l_, l_, st),
              "watfft deapply");

  const int ncnt = 2 + n_boxcars_;
  check_hip(hipMemsetAsync(row.counters, 0, ncnt * sizeof(unsigned), st),
            "memset counters");

  const uint8_t* ts_flags = nullptr;
  if (cfg_.enable_sk) {
    // 6. spectral kurtosis: row stats (fused into the backward DIF store
    //    when available — saves the 4 GB re-read) → flags → zap rows.
    //    sk_dif_partials exists only where the exec above was given it and
    //    its sums are those of the final waterfall (no window de-apply).
    if (fuse_into_bwd && s.sk_dif_partials)
      check_hip(sk_combine_partials(s.sk_dif_partials, s_,
                                    s.nbwd.dif_sk_wgs_per_row(), s.s2s4, st),
                "sk combine");
    else
      check_hip(sk_row_stats(wf, s_, l_, s.s2s4, st), "sk stats");
    check_hip(sk_flags(wf, s.s2s4, s_, l_, sk_lo_, sk_hi_, s.flags,
                       row.counters + 0, st),
              "sk flags");
    // NOTE: the waterfall itself is NOT zapped here — the time-series pass
    // below applies the flags directly, and zeroing the flagged rows of the
    // 4 GB waterfall (~1 ms/block) only matters when the waterfall is
    // actually read (product dump on detection, display).  waterfall_ptr()
    // performs the zap on demand.
    ts_flags = s.flags;
  }
  // 7. time series over non-zapped rows
  check_hip(time_series_2stage(wf, ts_flags, s_, l_, ts_count_, s.ts,
                               s.ts_partial, st),
            "ts");
  // 8. baseline subtract
  check_hip(sum_sumsq(s.ts, ts_count_, s.partials, s.sums, st), "ts sum");
  check_hip(subtract_mean(s.ts, ts_count_, s.sums, st), "ts sub");
  // 9. raw-series detection
  check_hip(sum_sumsq(s.ts, ts_count_, s.partials, s.sums, st), "ts var");
  check_hip(count_above(s.ts, ts_count_, s.sums + 1, cfg_.snr_threshold,
                        row.counters + 1, row.thresholds + 0, st),
            "count raw");
  // 10. boxcar ladder from the inclusive scan — fused: thresholds and
  // counts for every length derive directly from the ~1 MB cumulative sum
  // in 3 launches (was 3 per length; the box series never materialize)
  if (n_boxcars_ > 0) {
    check_hip(inclusive_scan(s.ts, s.cumsum, ts_count_, s.scan_scratch, st),
              "scan");
    check_hip(boxcar_ladder(s.cumsum, ts_count_, boxcar_lengths_.data(),
                            n_boxcars_, s.box_partials, cfg_.snr_threshold,
                            row.thresholds + 1, row.counters + 2, st),
              "box ladder");
  }
  // 11. result counters → pinned host
  check_hip(hipMemcpyAsync(row.h_counters, row.counters, ncnt * sizeof(unsigned),
                           hipMemcpyDeviceToHost, st),
            "res d2h");
  check_hip(hipMemcpyAsync(row.h_thresholds, row.thresholds,
                           (1 + n_boxcars_) * sizeof(float),
                           hipMemcpyDeviceToHost, st),
            "thr d2h");
  if (ts_dst)
    check_hip(hipMemcpyAsync(ts_dst, s.ts, ts_count_ * sizeof(float),
                             hipMemcpyDeviceToDevice, st),
              "ts plane row");
  s.last_row = row;
}

void PipelineEngine::check_trials(int n_trials) const {
  if (cfg_.max_dm_trials == 0)
    throw std::runtime_error(
        "submit_trials: the engine was built with max_dm_trials = 0");
  if (cfg_.use_phase_table)
    throw std::runtime_error(
        "submit_trials: DM trials need use_phase_table = false (the table "
        "holds one DM)");
  if (fuse_r2c_)
    throw std::runtime_error(
        "submit_trials: not supported with SRTB_FUSE_R2C=1 (the packed "
        "spectrum is not the retained r2c spectrum)");
  if (n_trials < 1 || n_trials > cfg_.max_dm_trials)
    throw std::runtime_error("submit_trials: n_trials = " +
                             std::to_string(n_trials) + " outside [1, " +
                             std::to_string(cfg_.max_dm_trials) + "]");
}

// One trial: backward half at trial k's DM from the retained spectrum into
// result row k and plane row k, then the peaks of its detection series.
void PipelineEngine::enqueue_trial(Slot& s, int k) {
  hipStream_t st = s.stream;
  const size_t nthr = 1 + (size_t)n_boxcars_;
  enqueue_back(s, s.trial_dms[k], trial_row(s, k),
               s.trial_plane + (size_t)k * ts_count_, /*keep_spectrum=*/true);
  check_hip(detect_peaks(s.ts, n_boxcars_ > 0 ? s.cumsum : nullptr, ts_count_,
                         boxcar_lengths_.data(), n_boxcars_, s.peak_scratch,
                         s.trial_peak_val + k * nthr,
                         s.trial_peak_idx + k * nthr, st),
            "detect peaks");
  check_hip(hipMemcpyAsync(s.h_trial_peak_val + k * nthr,
                           s.trial_peak_val + k * nthr, nthr * sizeof(float),
                           hipMemcpyDeviceToHost, st),
            "peak d2h");
  check_hip(hipMemcpyAsync(s.h_trial_peak_idx + k * nthr,
                           s.trial_peak_idx + k * nthr,
                           nthr * sizeof(unsigned), hipMemcpyDeviceToHost, st),
            "peak idx d2h");
  s.cur_trial = k;
}

void PipelineEngine::enqueue_trials(Slot& s, const uint8_t* dev_raw,
                                    const float* dev_samples,
                                    const double* dms, int n_trials) {
  RoctxRange r_chain("srtb_block_trials");
  s.trial_dms.assign(dms, dms + n_trials);
  bool any_poly = false;
  if (serial_chains_ < 0 && native_bwd_ && s.nbwd.first_pass_fusable())
    for (int k = 0; k < n_trials && !any_poly; ++k)
      any_poly = s.nbwd.preop_uses_poly(make_preop(s, dms[k]));
  order_after_last_chain(s, any_poly);
  enqueue_front(s, dev_raw, dev_samples);
  for (int k = 0; k < n_trials; ++k) enqueue_trial(s, k);
  check_hip(hipEventRecord(s.done, s.stream), "event record");
  s.busy = true;
  last_chain_done_ = s.done;
}

PipelineEngine::Slot& PipelineEngine::acquire_slot(int& id) {
  id = next_slot_;
  next_slot_ = (next_slot_ + 1) % n_slots_;
  Slot& s = *slots_[id];
  if (s.busy) {
    check_hip(hipEventSynchronize(s.done), "slot wait");
    s.busy = false;
  }
  return s;
}

int PipelineEngine::submit_trials(const void* host_bytes, size_t nbytes,
                                  const double* dms, int n_trials) {
  if (nbytes != raw_bytes_)
    throw std::runtime_error("submit_trials: wrong size");
  check_trials(n_trials);
  int id;
  Slot& s = acquire_slot(id);
  check_hip(hipMemcpyAsync(s.raw, host_bytes, nbytes, hipMemcpyHostToDevice,
                           s.stream),
            "raw h2d");
  enqueue_trials(s, s.raw, nullptr, dms, n_trials);
  return id;
}

int PipelineEngine::submit_trials_device(const void* dev_bytes, size_t nbytes,
                                         const double* dms, int n_trials,
                                         hipEvent_t wait_event) {
  if (nbytes != raw_bytes_)
    throw std::runtime_error("submit_trials: wrong size");
  check_trials(n_trials);
  int id;
  Slot& s = acquire_slot(id);
  if (wait_event)
    check_hip(hipStreamWaitEvent(s.stream, wait_event, 0), "producer wait");
  enqueue_trials(s, static_cast<const uint8_t*>(dev_bytes), nullptr, dms,
                 n_trials);
  return id;
}

int PipelineEngine::submit_trials_samples_device(const float* dev_samples,
                                                 size_t count,
                                                 const double* dms,
                                                 int n_trials,
                                                 hipEvent_t wait_event) {
  if (count != n_)
    throw std::runtime_error("submit_trials_samples: wrong count");
  check_trials(n_trials);
  int id;
  Slot& s = acquire_slot(id);
  if (wait_event)
    check_hip(hipStreamWaitEvent(s.stream, wait_event, 0), "fanout wait");
  enqueue_trials(s, nullptr, dev_samples, dms, n_trials);
  return id;
}

std::vector<TrialResult> PipelineEngine::wait_trials(int slot) {
  Slot& s = *slots_.at(slot);
  if (s.trial_dms.empty())
    throw std::runtime_error(
        "wait_trials: the slot's last submission carried no trials");
  check_hip(hipEventSynchronize(s.done), "wait trials");
  s.busy = false;
  s.wf_zap_pending = cfg_.enable_sk;  // see waterfall_ptr()
  const size_t ncnt = 2 + (size_t)n_boxcars_, nthr = 1 + (size_t)n_boxcars_;
  std::vector<TrialResult> out(s.trial_dms.size());
  for (size_t k = 0; k < out.size(); ++k) {
    TrialResult& t = out[k];
    const unsigned* c = s.h_trial_counters + k * ncnt;
    const float* thr = s.h_trial_thresholds + k * nthr;
    t.dm = s.trial_dms[k];
    t.result.zero_count = c[0];
    t.result.counts.emplace_back(1u, c[1]);
    for (int b = 0; b < n_boxcars_; ++b)
      t.result.counts.emplace_back((unsigned)boxcar_lengths_[b], c[2 + b]);
    t.result.thresholds.assign(thr, thr + nthr);
    for (size_t j = 0; j < nthr; ++j) {
      TrialPeak p;
      p.boxcar_length = j == 0 ? 1u : (unsigned)boxcar_lengths_[j - 1];
      p.value = s.h_trial_peak_val[k * nthr + j];
      p.index = s.h_trial_peak_idx[k * nthr + j];
      p.snr = p.value / (thr[j] / cfg_.snr_threshold);
      t.peaks.push_back(p);
    }
  }
  return out;
}

void PipelineEngine::select_trial(int slot, int k) {
  Slot& s = *slots_.at(slot);
  if (k < 0 || (size_t)k >= s.trial_dms.size())
    throw std::runtime_error(
        "select_trial: no such trial in the slot's last submission");
  if (k == s.cur_trial) return;
  enqueue_trial(s, k);
  check_hip(hipEventRecord(s.done, s.stream), "event record");
  s.busy = true;
  s.wf_zap_pending = cfg_.enable_sk;  // the new waterfall is not zapped yet
}

float* PipelineEngine::dm_time_plane_ptr(int slot) {
  Slot& s = *slots_.at(slot);
  if (!s.trial_plane)
    throw std::runtime_error("dm_time_plane: max_dm_trials = 0");
  return s.trial_plane;
}

int PipelineEngine::n_trials(int slot) const {
  return (int)slots_.at(slot)->trial_dms.size();
}


int PipelineEngine::submit(const void* host_bytes, size_t nbytes,
                           double dm_override) {
  if (nbytes != raw_bytes_) throw std::runtime_error("submit: wrong size");
  const int id = next_slot_;
  next_slot_ = (next_slot_ + 1) % n_slots_;
  Slot& s = *slots_[id];
  if (s.busy) {
    check_hip(hipEventSynchronize(s.done), "slot wait");
    s.busy = false;
  }
  if (fold_v_) stamp_fold(s);
  const bool graph_ok = cfg_.use_hip_graph && std::isnan(dm_override);
  if (graph_ok && s.graph_exec && s.graph_host_src == host_bytes) {
    // steady state: replay the captured chain (H2D + kernels + D2H)
    check_hip(hipGraphLaunch(s.graph_exec, s.stream), "graph launch");
    check_hip(hipEventRecord(s.done, s.stream), "event record");
    s.busy = true;
    s.last_row = plain_row(s);  // a trial submission may have come between
    s.trial_dms.clear();
    s.cur_trial = -1;
    return id;
  }
  if (graph_ok && s.graph_pending >= 1 && !s.graph_exec) {
    // second submission from the same host buffer: capture it
    check_hip(hipStreamBeginCapture(s.stream, hipStreamCaptureModeThreadLocal),
              "begin capture");
    check_hip(hipMemcpyAsync(s.raw, host_bytes, nbytes,
                             hipMemcpyHostToDevice, s.stream),
              "raw h2d");
    enqueue_chain(s, s.raw, nullptr, dm_override, /*record_event=*/false);
    hipGraph_t g = nullptr;
    check_hip(hipStreamEndCapture(s.stream, &g), "end capture");
    check_hip(hipGraphInstantiate(&s.graph_exec, g, nullptr, nullptr, 0),
              "graph instantiate");
    check_hip(hipGraphDestroy(g), "graph destroy");
    s.graph_host_src = host_bytes;
    check_hip(hipGraphLaunch(s.graph_exec, s.stream), "graph launch");
    check_hip(hipEventRecord(s.done, s.stream), "event record");
    s.busy = true;
    return id;
  }
  if (graph_ok) {
    s.graph_pending = 1;
    s.graph_host_src = host_bytes;
  }
  check_hip(hipMemcpyAsync(s.raw, host_bytes, nbytes, hipMemcpyHostToDevice,
                           s.stream),
            "raw h2d");
  enqueue_chain(s, s.raw, nullptr, dm_override);
  return id;
}

int PipelineEngine::submit_device(const void* dev_bytes, size_t nbytes,
                                  double dm_override, hipEvent_t wait_event) {
  if (nbytes != raw_bytes_) throw std::runtime_error("submit: wrong size");
  const int id = next_slot_;
  next_slot_ = (next_slot_ + 1) % n_slots_;
  Slot& s = *slots_[id];
  if (s.busy) {
    check_hip(hipEventSynchronize(s.done), "slot wait");
    s.busy = false;
  }
  if (fold_v_) stamp_fold(s);
  if (wait_event)
    check_hip(hipStreamWaitEvent(s.stream, wait_event, 0), "producer wait");
  enqueue_chain(s, static_cast<const uint8_t*>(dev_bytes), nullptr,
                dm_override);
  return id;
}

int PipelineEngine::submit_samples_device(const float* dev_samples,
                                          size_t count, double dm_override,
                                          hipEvent_t wait_event) {
  if (count != n_) throw std::runtime_error("submit_samples: wrong count");
  const int id = next_slot_;
  next_slot_ = (next_slot_ + 1) % n_slots_;
  Slot& s = *slots_[id];
  if (s.busy) {
    check_hip(hipEventSynchronize(s.done), "slot wait");
    s.busy = false;
  }
  if (fold_v_) stamp_fold(s);
  if (wait_event)
    check_hip(hipStreamWaitEvent(s.stream, wait_event, 0), "fanout wait");
  enqueue_chain(s, nullptr, dev_samples, dm_override);
  return id;
}

BlockResult PipelineEngine::wait(int slot) {
  Slot& s = *slots_.at(slot);
  check_hip(hipEventSynchronize(s.done), "wait");
  s.busy = false;
  s.wf_zap_pending = cfg_.enable_sk;  // see waterfall_ptr()
  BlockResult r;
  // the plain row, or after a trial submission the row of the last trial run
  const unsigned* hc = s.last_row.h_counters;
  const float* ht = s.last_row.h_thresholds;
  r.zero_count = hc[0];
  r.counts.emplace_back(1u, hc[1]);
  for (int b = 0; b < n_boxcars_; ++b)
    r.counts.emplace_back((unsigned)boxcar_lengths_[b], hc[2 + b]);
  r.thresholds.assign(ht, ht + 1 + n_boxcars_);
  return r;
}

void PipelineEngine::synchronize() {
  for (auto& sp : slots_) {
    check_hip(hipStreamSynchronize(sp->stream), "sync");
    sp->busy = false;
  }
}

float2* PipelineEngine::waterfall_ptr(int slot) {
  Slot& s = *slots_.at(slot);
  float2* wf = s.wf ? s.wf : s.spec;
  if (s.wf_zap_pending) {
    // deferred SK row zap (flags are still resident for this slot); only
    // blocks whose waterfall is actually consumed pay the 4 GB pass
    check_hip(sk_zap_rows(wf, s.flags, s_, l_, s.stream), "sk zap lazy");
    check_hip(hipStreamSynchronize(s.stream), "sk zap sync");
    s.wf_zap_pending = false;
  }
  return wf;
}
const float2* PipelineEngine::waterfall_unzapped_ptr(int slot) const {
  const Slot& s = *slots_.at(slot);
  return s.wf ? s.wf : s.spec;
}
const float2* PipelineEngine::sk_stats_ptr(int slot) const {
  return cfg_.enable_sk ? slots_.at(slot)->s2s4 : nullptr;
}
const uint8_t* PipelineEngine::sk_flags_ptr(int slot) const {
  return cfg_.enable_sk ? slots_.at(slot)->flags : nullptr;
}
float* PipelineEngine::time_series_ptr(int slot) { return slots_.at(slot)->ts; }
float* PipelineEngine::cumsum_ptr(int slot) { return slots_.at(slot)->cumsum; }
hipStream_t PipelineEngine::stream(int slot) { return slots_.at(slot)->stream; }

const void* PipelineEngine::filterbank_host(int slot) {
  Slot& s = *slots_.at(slot);
  if (!s.h_fil) throw std::runtime_error("filterbank: fil_tscrunch = 0");
  return s.h_fil;
}

float* PipelineEngine::filterbank_power_ptr(int slot) {
  Slot& s = *slots_.at(slot);
  if (!s.fil_power) throw std::runtime_error("filterbank: fil_tscrunch = 0");
  return s.fil_power;
}

const float* PipelineEngine::filterbank_mean_host(int slot) {
  Slot& s = *slots_.at(slot);
  if (!s.h_fil_stats)
    throw std::runtime_error("filterbank: statistics exist only at 8 bits");
  return s.h_fil_stats;
}

const float* PipelineEngine::filterbank_std_host(int slot) {
  return filterbank_mean_host(slot) + fil_c_;
}

float* PipelineEngine::compute_boxcar(int slot, size_t L) {
  float* box = compute_boxcar_async(slot, L);
  check_hip(hipStreamSynchronize(slots_.at(slot)->stream), "boxcar sync");
  return box;
}

float* PipelineEngine::compute_boxcar_async(int slot, size_t L) {
  Slot& s = *slots_.at(slot);
  const size_t n_out = ts_count_ - L;
  check_hip(boxcar(s.cumsum, s.box, n_out, L, s.stream), "boxcar recompute");
  return s.box;
}

}  // namespace srtb_hip
