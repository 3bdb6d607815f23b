// IncoherentSearch — searches DM offsets around the engine's one coherent DM
// on the stream of filterbank power planes (docs/ARCHITECTURE.md, "Incoherent
// DM-offset search").  It keeps the last D_max + R plane rows in a device
// ring, dedisperses every block at all offsets into a [T][R] DM-time plane
// and runs the boxcar detection on every trial, all on its own non-blocking
// stream.  No host synchronization on submit: the stream waits on an event
// recorded on the producer's stream.
//
// Blocks are submitted in stream order on the one stream, which is what makes
// the history well-defined across the engine's slots.
//
// Contract: after submit(engine, slot) returned k, the engine slot is not
// resubmitted before wait(k) has returned — the copy reads the slot's plane
// in place.

#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>
#include <vector>

#include "engine.h"

namespace srtb_hip {

struct IncoherentSearchConfig {
  size_t rows = 0;      // R, plane rows per block
  size_t channels = 0;  // C
  double fch1 = 0;      // MHz, centre of channel 0
  double foff = 0;      // MHz per channel (negative: descending frequency)
  double tsamp = 0;     // seconds per plane row
  std::vector<double> offsets;  // delta_t, pc cm^-3, either sign
  double snr_threshold = 6.0;
  size_t max_boxcar = 1;
  // per-channel normalisation of the rows entering the history, by a running
  // mean and deviation over about normalize_blocks blocks (1 .. 65536)
  bool normalize = false;
  size_t normalize_blocks = 8;
};

// d[t][c] of the definition, built in fp64; throws on non-finite input
std::vector<int32_t> incoherent_delays(double fch1, double foff, size_t C,
                                       double tsamp,
                                       const std::vector<double>& offsets);

struct IncoherentDetection {
  size_t boxcar_length = 0;
  double peak = 0;
  uint32_t index = 0;  // UINT_MAX: the length has no window
  double rms = 0;
  uint32_t count = 0;
  double snr = 0;  // peak / rms, 0 where rms = 0
};

struct IncoherentTrial {
  double offset = 0;  // delta_t
  double mean = 0;    // mu
  std::vector<IncoherentDetection> lengths;
};

struct IncoherentResult {
  bool valid = false;     // block * R >= D_max; trials is empty otherwise
  int64_t first_row = 0;  // global row of Y[.][0] = block * R - D_max
  uint64_t block = 0;     // ordinal since construction / reset()
  // channels with a gain > 0 in this block, valid or not (0 with
  // normalize off)
  uint32_t live_channels = 0;
  std::vector<IncoherentTrial> trials;
};

class IncoherentSearch {
 public:
  explicit IncoherentSearch(const IncoherentSearchConfig& cfg,
                            int n_slots = 2);
  ~IncoherentSearch();
  IncoherentSearch(const IncoherentSearch&) = delete;
  IncoherentSearch& operator=(const IncoherentSearch&) = delete;

  // Call after the engine's submit, without waiting for it.  Blocks only
  // while the searcher's own next slot (round-robin) is still in flight.
  // Throws if the engine's filterbank geometry differs.  Returns the slot.
  int submit(PipelineEngine& eng, int slot);
  // The same from any device plane [R][C]; `ready` (nullable) is an event
  // already recorded on the stream that produces it.
  int submit_plane(const float* dev_plane, hipEvent_t ready);

  // One hipEventSynchronize on the slot's `done` event.
  IncoherentResult wait(int k);

  // Zeroes the history and the normalisation state and restarts priming
  // (after dropped blocks).
  void reset();

  size_t rows() const { return cfg_.rows; }
  size_t channels() const { return cfg_.channels; }
  size_t trials() const { return cfg_.offsets.size(); }
  int n_lengths() const { return nl_; }
  int n_slots() const { return (int)slots_.size(); }
  size_t d_max() const { return d_max_; }
  const std::vector<int32_t>& delays() const { return delays_; }  // [T][C]
  const std::vector<double>& offsets() const { return cfg_.offsets; }
  float* plane_ptr(int k) const;         // device Y [T][R]
  const float* plane_host(int k) const;  // pinned mirror, after wait(k)
  // The running state of the normalisation, device [C]; null with normalize
  // off.  Written on stream(): synchronize it before reading.
  bool normalize() const { return cfg_.normalize; }
  const double* norm_mean() const { return norm_m_; }
  const double* norm_var() const { return norm_v_; }
  const float* norm_gain() const { return norm_g_; }
  hipStream_t stream() const { return stream_; }

 private:
  struct Slot {
    float* y = nullptr;        // [T][R]
    double* res_f64 = nullptr;  // peak [T][NL], rms [T][NL], mu [T]
    // index [T][NL], count [T][NL]; with normalize, live [1] after them
    unsigned* res_u32 = nullptr;
    float* h_y = nullptr;
    double* h_f64 = nullptr;
    unsigned* h_u32 = nullptr;
    hipEvent_t ready = nullptr, done = nullptr;
    bool busy = false, valid = false;
    int64_t first_row = 0;
    uint64_t block = 0;
  };
  IncoherentSearchConfig cfg_;
  std::vector<int32_t> delays_;
  size_t d_max_ = 0, ring_rows_ = 0, write_row_ = 0;
  uint64_t block_ = 0;
  int nl_ = 0;
  float* ring_ = nullptr;      // [D_max + R][C]
  int* d_delays_ = nullptr;    // [T][C]
  float* partials_ = nullptr;  // shared: the one stream serializes the blocks
  // normalisation (allocated with cfg_.normalize only): running mean and
  // variance, gain, scratch of the block statistics
  double* norm_m_ = nullptr;   // [C], norm_v_ follows it in one allocation
  double* norm_v_ = nullptr;   // [C]
  float* norm_g_ = nullptr;    // [C]
  double* norm_partials_ = nullptr;
  hipStream_t stream_ = nullptr;
  std::vector<Slot> slots_;
  int next_slot_ = 0;
};

}  // namespace srtb_hip
