// PolCombiner — joins the two per-polarization engines of a dual-polarization
// stream on the GPU: after both engines' submissions it reads their two
// coherently dedispersed waterfalls once and leaves the block's polarization
// products (docs/ARCHITECTURE.md, "Polarization products") as a [R][P][C]
// plane in pinned host memory.  No host synchronization: the combiner's own
// stream waits on an event recorded on each engine's slot stream.
//
// Contract: after submit(a, slot_a, b, slot_b) returned k, neither engine slot
// is resubmitted before wait(k) has returned — the kernel reads the slots'
// waterfalls and flags in place.

#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>
#include <memory>
#include <vector>

#include "engine.h"

namespace srtb_hip {

struct PolCombinerConfig {
  size_t baseband_input_count = 0;    // N real samples per block and engine
  size_t spectrum_channel_count = 0;  // S
  size_t nsamps_reserved = 0;         // overlap (real samples)
  size_t tscrunch = 16;  // power of two <= kFilterbankMaxTscrunch
  size_t fscrunch = 1;   // divides S
  bool reverse = false;  // descending-frequency output (bandwidth > 0)
  int pol_state = kPolStateIQUV;
  int nbits = 32;  // 8 (per-block, per-(product, channel) uint8) or 32
};

class PolCombiner {
 public:
  explicit PolCombiner(const PolCombinerConfig& cfg, int n_slots = 2);
  ~PolCombiner();
  PolCombiner(const PolCombiner&) = delete;
  PolCombiner& operator=(const PolCombiner&) = delete;

  // Call after both engines' submits, without waiting for them.  Blocks only
  // while the combiner's own next slot (round-robin) is still in flight.
  // Throws if the engines' n(), n_channels() or waterfall_len() differ from
  // each other or from the combiner's geometry.  Returns the slot used.
  int submit(PipelineEngine& a, int slot_a, PipelineEngine& b, int slot_b);

  // One hipEventSynchronize on the slot's `done` event.
  void wait(int k);

  size_t rows() const { return r_; }
  size_t channels() const { return c_; }
  int nifs() const { return p_; }
  int nbits() const { return cfg_.nbits; }
  int n_slots() const { return (int)slots_.size(); }
  // pinned mirrors, complete after wait(k) and valid until slot k is used
  // again: host = [rows][nifs][channels] uint8 or float, mean/std =
  // [nifs * channels] float (8-bit only, otherwise they throw)
  const void* host(int k) const;
  float* power_ptr(int k) const;  // device float [rows][nifs][channels]
  const float* mean_host(int k) const;
  const float* std_host(int k) const;

 private:
  struct Slot {
    float* power = nullptr;      // [R][P][C]
    float* stats = nullptr;      // [2][P*C] mean, std (8-bit)
    uint8_t* u8 = nullptr;       // [R][P][C] (8-bit)
    double* partials = nullptr;  // stats scratch (8-bit)
    void* h_plane = nullptr;     // pinned mirror of the output plane
    float* h_stats = nullptr;    // pinned [2][P*C] (8-bit)
    hipEvent_t ready_a = nullptr, ready_b = nullptr, done = nullptr;
    bool busy = false;
  };
  PolCombinerConfig cfg_;
  size_t l_ = 0, v_ = 0, r_ = 0, c_ = 0;
  int p_ = 0;
  hipStream_t stream_ = nullptr;
  std::vector<Slot> slots_;
  int next_slot_ = 0;
};

}  // namespace srtb_hip
