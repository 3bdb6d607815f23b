// PipelineEngine — the MI355X-native per-GPU streaming engine.
//
// Runs the full per-block chain of the reference's streaming data path
//  with zero host synchronization inside a block:
//
//   H2D(raw) → unpack(+window) → R2C FFT → mean-power reduce →
//   fused {RFI-s1 zap + normalize + manual zap + coherent dedispersion} →
//   batched backward C2C (waterfall) → SK row stats → flags → zap rows →
//   time series → baseline subtract → threshold counts → prefix scan →
//   boxcar ladder (2,4,…,max) with per-length thresholds →
//   D2H(result counters) → [filterbank: detect → stats → quantise → D2H] →
//   [fold: phase words H2D → turn table → counts → accumulate] → event
//
// Two slots, each with its own HIP stream, device buffers and hipFFT plans:
// while slot A computes, slot B's next block uploads (the reference instead
// waits after every kernel — SURVEY.md §2b note).  Results (detection
// counters) land in pinned memory; wait(slot) is the only host sync.

#pragma once

#include <hip/hip_runtime.h>

#include <array>
#include <cstdint>
#include <memory>
#include <vector>

#include "../fft/fft_plans.h"
#include "../fft/native_fft.h"
#include "../include/srtb_kernels.h"

namespace srtb_hip {

struct EngineConfig {
  size_t baseband_input_count = 1ull << 28;  // N real samples per block
  int baseband_input_bits = 8;               // 1/2/4/8/-8/16/-16/32/-32
  size_t spectrum_channel_count = 1ull << 15;  // S
  double freq_low = 1000.0;    // MHz
  double bandwidth = 500.0;    // MHz (may be negative)
  double sample_rate = 1e9;    // samples/s
  double dm = 0.0;
  float rfi_threshold = 10.0f;          // mitigate_rfi_average_method_threshold
  float sk_threshold = 1.1f;            // mitigate_rfi_spectral_kurtosis_threshold
  float snr_threshold = 6.0f;           // signal_detect_signal_noise_threshold
  size_t max_boxcar_length = 1024;
  size_t nsamps_reserved = 0;           // overlap (real samples), from host
  int n_zap_ranges = 0;
  ZapRange zap_ranges[16] = {};
  bool use_phase_table = false;  // cache dedispersion factors for fixed DM
  bool enable_rfi_s1 = true;
  bool enable_sk = true;
  // 0 = native always, 1 = hipFFT always, 2 = auto (native forward; the
  // batched backward picks rocFFT below the measured 2^17 crossover —
  // rocFFT's specialized sbcc/sbrc kernels win 1.4-2.9x for lengths
  // ≤ 2^16, the native column+DIF plan wins 2.2x at 2^18)
  int fft_backend = 2;
  // FFT window fused into unpack: 0 = rectangle (reference default),
  // 1 = hann, 2 = hamming
  int window_kind = 0;
  // capture the steady-state per-block chain (~55 launches) into a hipGraph
  // per slot and replay it; falls back to direct enqueue whenever the
  // submission differs from the captured one (dm override, other host ptr)
  bool use_hip_graph = false;
  // DM-trial search (submit_trials): the largest number of trials one
  // submission may carry.  0 = the mode is off and nothing is allocated;
  // T > 0 adds per slot one [Nc] work buffer, a [T][ts_count] DM-time plane
  // and T result rows.  At most kMaxDmTrials.
  int max_dm_trials = 0;
  // Filterbank output (docs/ARCHITECTURE.md): every block's waterfall is
  // reduced to a [R][C] power plane that lands in pinned host memory before
  // the slot's `done` event.  fil_tscrunch = 0 = off, nothing is allocated.
  // tscrunch, fscrunch: powers of two, tscrunch <= 4096, fscrunch divides S;
  // (N - nsamps_reserved) must be a multiple of 2*S*tscrunch.  nbits: 8
  // (per-block, per-channel normalised uint8) or 32 (float power).  Not
  // together with max_dm_trials > 0.
  size_t fil_tscrunch = 0;
  size_t fil_fscrunch = 1;
  int fil_nbits = 32;
  // Pulsar folding (docs/ARCHITECTURE.md): every block's waterfall is folded
  // into per-slot fp64 [S][fold_nbin] profiles at spin frequency fold_f0 (Hz),
  // derivative fold_f1 (Hz/s) and phase fold_phase0 (turns at stream sample
  // 0).  fold_nbin = 0 = off, nothing is allocated; otherwise 2..65536,
  // fold_f0 > 0 with fold_f0 * 2S / sample_rate < 1, and
  // (N - nsamps_reserved) a multiple of 2S.  Not together with
  // max_dm_trials > 0.
  size_t fold_nbin = 0;
  double fold_f0 = 0.0;
  double fold_f1 = 0.0;
  double fold_phase0 = 0.0;
};

constexpr int kMaxDmTrials = 256;

struct BlockResult {
  unsigned zero_count = 0;  // zapped-channel count (gate detections on host)
  // (boxcar_length, signal_count) — boxcar_length 1 is the raw series
  std::vector<std::pair<unsigned, unsigned>> counts;
  std::vector<float> thresholds;
};

// Peak of one detection series of one trial: the maximum, the lowest sample
// index attaining it (boxcar's indexing: the window starts after `index`) and
// the maximum in units of the rms the detection threshold is built from,
// snr = value / (threshold / snr_threshold).
struct TrialPeak {
  unsigned boxcar_length = 1;  // 1 = the raw series
  float value = 0;
  unsigned index = 0;
  float snr = 0;
};

struct TrialResult {
  double dm = 0;
  BlockResult result;
  std::vector<TrialPeak> peaks;  // raw series, then one per ladder length
};

class PipelineEngine {
 public:
  explicit PipelineEngine(const EngineConfig& cfg, int n_slots = 2);
  ~PipelineEngine();
  PipelineEngine(const PipelineEngine&) = delete;
  PipelineEngine& operator=(const PipelineEngine&) = delete;

  // Upload raw bytes (host, ideally pinned) and enqueue the whole chain on
  // the slot's stream.  Blocks only if the slot's previous block is still in
  // flight.  Returns the slot used.
  // dm_override: NAN = use the configured DM; a finite value re-runs the
  // (on-the-fly fp64) dedispersion at that DM — the DM-trial sweep path.
  int submit(const void* host_bytes, size_t nbytes, double dm_override = NAN);

  // Enqueue the chain reading raw bytes already on the device (e.g. from a
  // torch tensor); caller guarantees lifetime until wait().  wait_event
  // (optional): slot stream waits on it first — pass an event recorded on
  // the stream that produced dev_bytes (e.g. torch's current stream).
  int submit_device(const void* dev_bytes, size_t nbytes,
                    double dm_override = NAN, hipEvent_t wait_event = nullptr);

  // Enqueue the chain starting at the R2C FFT from already-unpacked float
  // samples on the device (count = baseband_input_count).  Used for
  // multi-polarization formats whose unpack fans one packet stream out into
  // several sample streams (reference unpack_pipe.hpp:146-390).
  // The chain starts at the FFT, so the FFT window is the caller's job: with
  // window_kind != 0 pass samples already multiplied by
  // build_window(count, window_kind) (the unpack launchers take it), because
  // the engine still de-applies the waterfall window after the backward FFT.
  // wait_event (optional): the slot's stream waits on it before the chain —
  // lets an app-owned fan-out stream (H2D + unpack of the packed block)
  // feed several engines without host synchronization.
  int submit_samples_device(const float* dev_samples, size_t count,
                            double dm_override = NAN,
                            hipEvent_t wait_event = nullptr);

  // DM-trial search: ONE forward half (unpack, forward FFT, r2c finish,
  // mean power) per block, then one backward half per trial DM, each from
  // the block's forward spectrum, which stays intact in the slot.  Trial k
  // fills result row k and row k of the DM-time plane and is followed by the
  // peak search.  Everything runs on the slot's stream with one `done` event
  // at the end; never through the hipGraph path.  Needs max_dm_trials > 0
  // and use_phase_table = false; 1 <= n_trials <= max_dm_trials.
  int submit_trials(const void* host_bytes, size_t nbytes, const double* dms,
                    int n_trials);
  int submit_trials_device(const void* dev_bytes, size_t nbytes,
                           const double* dms, int n_trials,
                           hipEvent_t wait_event = nullptr);
  int submit_trials_samples_device(const float* dev_samples, size_t count,
                                   const double* dms, int n_trials,
                                   hipEvent_t wait_event = nullptr);

  // Wait for a slot's chain and return its detection counters.  After a
  // trial submission: those of the trial most recently run.
  BlockResult wait(int slot);

  // Wait for a slot's trial submission and return every trial's result.
  std::vector<TrialResult> wait_trials(int slot);

  // Re-run trial k's backward half from the retained spectrum on the slot's
  // stream (asynchronous; rewrites result row k and plane row k with the same
  // values) so that waterfall_ptr, time_series_ptr, cumsum_ptr and
  // compute_boxcar* refer to trial k.  No-op when k was the last trial run.
  // Valid until the slot is submitted again.
  void select_trial(int slot, int k);

  // [n_trials(slot)][ts_count] baseline-subtracted series, one row per trial.
  float* dm_time_plane_ptr(int slot);
  int n_trials(int slot) const;  // trials of the slot's last submission

  // Wait for all outstanding work.
  void synchronize();

  // Geometry
  size_t n() const { return n_; }
  size_t nc() const { return nc_; }
  size_t n_channels() const { return s_; }
  size_t waterfall_len() const { return l_; }
  size_t ts_count() const { return ts_count_; }
  size_t raw_bytes() const { return raw_bytes_; }
  int n_boxcars() const { return n_boxcars_; }
  int n_slots() const { return n_slots_; }

  // Device pointers of a slot (valid after wait(slot)) — for tests, dumps and
  // the display path.
  float2* waterfall_ptr(int slot);   // [S][L]
  // Test surface: the waterfall as the chain left it (waterfall_ptr without
  // the deferred row zap) and the spectral-kurtosis products of the slot's
  // last back half; sk_* are null with enable_sk = false.
  const float2* waterfall_unzapped_ptr(int slot) const;
  const float2* sk_stats_ptr(int slot) const;  // [S] <sum|x|^2, sum|x|^4>
  const uint8_t* sk_flags_ptr(int slot) const;  // [S]
  float* time_series_ptr(int slot);  // [ts_count]
  float* cumsum_ptr(int slot);       // [ts_count]
  // Recompute one boxcar series into the slot's boxcar buffer and return it
  // (for dumping a detected series).
  float* compute_boxcar(int slot, size_t boxcar_length);
  // Async variant: enqueue the recompute on the slot's stream and return the
  // device pointer WITHOUT synchronizing (follow with hipMemcpyAsync on the
  // same stream + an event for a fully async detection dump).
  float* compute_boxcar_async(int slot, size_t boxcar_length);

  hipStream_t stream(int slot);

  // Filterbank output (fil_tscrunch > 0; otherwise rows = channels = 0 and
  // the pointer accessors throw).  The host pointers are the slot's pinned
  // mirrors, complete after wait(slot) and valid until the slot is submitted
  // again: filterbank_host = [rows][channels] uint8 or float, mean/std =
  // [channels] float (8-bit only).
  size_t filterbank_rows() const { return fil_r_; }
  size_t filterbank_channels() const { return fil_c_; }
  int filterbank_nbits() const { return fil_r_ ? cfg_.fil_nbits : 0; }
  const void* filterbank_host(int slot);
  float* filterbank_power_ptr(int slot);  // device [rows][channels]
  const float* filterbank_mean_host(int slot);
  const float* filterbank_std_host(int slot);

  // Pulsar folding (fold_nbin > 0; otherwise fold_read and fold_reset throw).
  // The engine keeps a running stream position: every plain submission
  // (submit, submit_device, submit_samples_device) folds with it as the index
  // n0 of the block's first real sample, then advances it by
  // N - nsamps_reserved.  set_fold_next_sample overrides it for the next
  // submission (dropped blocks, multi-rank replay).
  struct FoldWords {
    uint64_t n0 = 0, phi = 0, dphi = 0;  // of a slot's last submission
  };
  size_t fold_nbin() const { return cfg_.fold_nbin; }
  size_t fold_valid() const { return fold_v_; }
  void set_fold_next_sample(uint64_t n0) { fold_pos_ = n0; }
  uint64_t fold_next_sample() const { return fold_pos_; }
  FoldWords fold_words(int slot) const;
  // Synchronises the whole engine (every slot's stream), then returns the
  // slots' accumulators summed in slot order: acc [S][nbin], hits [nbin],
  // weights [S].  Meant for sub-integration boundaries, not for every block.
  void fold_read(double* acc, uint64_t* hits, uint64_t* weights);
  // Synchronises, zeroes the accumulators; the stream position stays.
  void fold_reset();

 private:
  struct Slot;
  // where one backward half leaves its counters and thresholds
  struct ResultRow {
    unsigned* counters = nullptr;    // device [2 + n_boxcars]
    float* thresholds = nullptr;     // device [1 + n_boxcars]
    unsigned* h_counters = nullptr;  // pinned mirrors
    float* h_thresholds = nullptr;
  };
  void enqueue_chain(Slot& s, const uint8_t* dev_raw,
                     const float* dev_samples, double dm,
                     bool record_event = true);
  // the chain's two halves, see engine.cpp
  void enqueue_front(Slot& s, const uint8_t* dev_raw,
                     const float* dev_samples);
  void enqueue_back(Slot& s, double dm, const ResultRow& row, float* ts_dst,
                    bool keep_spectrum);
  FftPreop make_preop(const Slot& s, double dm) const;
  void order_after_last_chain(Slot& s, bool uses_poly);
  ResultRow plain_row(Slot& s) const;
  ResultRow trial_row(Slot& s, int k) const;
  Slot& acquire_slot(int& id);
  void enqueue_trials(Slot& s, const uint8_t* dev_raw,
                      const float* dev_samples, const double* dms,
                      int n_trials);
  void enqueue_trial(Slot& s, int k);
  void check_trials(int n_trials) const;
  void enqueue_filterbank(Slot& s);
  void stamp_fold(Slot& s);
  void enqueue_fold(Slot& s);

  EngineConfig cfg_;
  size_t n_, nc_, s_, l_, ts_count_, raw_bytes_;
  // filterbank geometry: valid waterfall columns, output rows and channels
  size_t fil_v_ = 0, fil_r_ = 0, fil_c_ = 0;
  // folding: valid waterfall columns, phase step per real sample (2^64 = one
  // turn), index in the stream of the next block's first sample
  size_t fold_v_ = 0;
  uint64_t fold_step_ = 0;
  uint64_t fold_pos_ = 0;
  int n_boxcars_ = 0;
  std::vector<size_t> boxcar_lengths_;
  float sk_lo_ = 0, sk_hi_ = 0;
  float norm_coeff_ = 1.0f;
  double f_min_ = 0, f_c_ = 0, df_ = 0;
  int n_slots_ = 2;

  float2* phase_table_ = nullptr;  // shared across slots (read-only)
  float* window_ = nullptr;        // fused FFT window table (null = rect)
  float* watfft_window_ = nullptr;  // K21 de-apply table, length l_
  bool native_fft_ = false;        // hand-written FORWARD FFT active
  bool fused_unpack_off_ = false;  // SRTB_NO_FUSED_UNPACK kill switch
  bool native_bwd_ = false;        // hand-written BACKWARD (waterfall) FFT
  bool fuse_r2c_ = false;          // r2c pair-combine fused into bwd load
  size_t fwd_pw_n_ = 0;            // fwd power partial count


  struct Slot {
    hipStream_t stream = nullptr;
    hipEvent_t done = nullptr;
    bool busy = false;
    bool wf_zap_pending = false;    // SK zap deferred until waterfall read
    float2* wf = nullptr;           // where the waterfall landed last block
    uint8_t* raw = nullptr;         // device raw bytes
    float* samples = nullptr;       // [N] unpacked
    float2* spec = nullptr;         // [Nc+1] spectrum / waterfall (in-place)
    float2* xbuf = nullptr;         // [Nc] bwd working set (r2c fusion)
    float2* fwd_pw = nullptr;       // fwd-DIF per-WG power partials
    double* r2c_final_partials = nullptr;  // fused r2c store's mean partials
                                           // (non-null = that path is taken)
    float2* s2s4 = nullptr;         // [S]
    float2* sk_dif_partials = nullptr;  // [S * wgs_per_row] (fused SK stats)
    uint8_t* flags = nullptr;       // [S]
    float* ts = nullptr;            // [ts_count]
    float* ts_partial = nullptr;    // [chunks][ts_count] two-stage scratch
    float* cumsum = nullptr;        // [ts_count]
    float* box = nullptr;           // [ts_count]
    float* scan_scratch = nullptr;  // [4096]
    double* partials = nullptr;     // reduce partials + out scalars
    double* box_partials = nullptr; // [n_boxcars][2][reduce_partials]
    double* mean_power = nullptr;   // -> inside partials block
    double* sums = nullptr;         // [2]
    unsigned* counters = nullptr;   // [1 + n_boxcars + 1] zero_count + counts
    float* thresholds = nullptr;    // [1 + n_boxcars]
    unsigned* h_counters = nullptr; // pinned result mirror
    float* h_thresholds = nullptr;  // pinned
    FftPlanSet plans;               // hipFFT fallback
    NativeFft nfwd, nbwd;           // hand-written path
    // hipGraph replay state
    hipGraphExec_t graph_exec = nullptr;
    const void* graph_host_src = nullptr;  // host ptr the capture used
    int graph_pending = 0;  // submissions seen for this slot
    // DM-trial state (allocated only with max_dm_trials > 0)
    float2* trial_w = nullptr;        // [Nc] per-trial backward working set
    float* trial_plane = nullptr;     // [T][ts_count]
    unsigned* trial_counters = nullptr;   // [T][2 + n_boxcars]
    float* trial_thresholds = nullptr;    // [T][1 + n_boxcars]
    float* trial_peak_val = nullptr;      // [T][1 + n_boxcars]
    unsigned* trial_peak_idx = nullptr;   // [T][1 + n_boxcars]
    unsigned* h_trial_counters = nullptr;  // pinned mirrors of the four
    float* h_trial_thresholds = nullptr;
    float* h_trial_peak_val = nullptr;
    unsigned* h_trial_peak_idx = nullptr;
    void* peak_scratch = nullptr;
    std::vector<double> trial_dms;  // of the last trial submission
    int cur_trial = -1;             // trial whose products the slot holds
    ResultRow last_row;             // row of the back half most recently run
    // filterbank state (allocated only with fil_tscrunch > 0)
    float* fil_power = nullptr;       // [R][C]
    float* fil_stats = nullptr;       // [2][C] mean, std (8-bit)
    uint8_t* fil_u8 = nullptr;        // [R][C] (8-bit)
    double* fil_partials = nullptr;   // stats scratch (8-bit)
    void* h_fil = nullptr;            // pinned mirror of the output plane
    float* h_fil_stats = nullptr;     // pinned [2][C] (8-bit)
    // folding state (allocated only with fold_nbin > 0)
    double* fold_acc = nullptr;         // [S][nbin]
    uint64_t* fold_hits = nullptr;      // [nbin]
    uint64_t* fold_weights = nullptr;   // [S]
    uint64_t* fold_dwords = nullptr;    // device {Phi_b, dPhi_b}
    uint64_t* h_fold_words = nullptr;   // pinned source of fold_dwords
    uint32_t* fold_table = nullptr;     // turn table scratch
    FoldWords fold_last;
  };
  std::vector<std::unique_ptr<Slot>> slots_;
  int next_slot_ = 0;
  // `done` event of the most recently enqueued chain (any slot): the next
  // chain waits on it when chains are serialized, see enqueue_chain()
  hipEvent_t last_chain_done_ = nullptr;
  int serial_chains_ = -1;  // SRTB_SERIAL_CHAINS: -1 auto, 0 never, 1 always
};

}  // namespace srtb_hip
