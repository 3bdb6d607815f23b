// PolCombiner implementation (see pol_combiner.h).

#include "pol_combiner.h"

#include <stdexcept>
#include <string>

namespace srtb_hip {

PolCombiner::PolCombiner(const PolCombinerConfig& cfg, int n_slots)
    : cfg_(cfg) {
  auto pow2 = [](size_t x) { return x && !(x & (x - 1)); };
  const size_t n = cfg.baseband_input_count, s = cfg.spectrum_channel_count;
  const size_t t = cfg.tscrunch, f = cfg.fscrunch;
  if (n_slots < 1) throw std::runtime_error("pol combiner: n_slots must be >= 1");
  if (s == 0 || n == 0 || n % (2 * s) != 0)
    throw std::runtime_error(
        "pol combiner: baseband_input_count must be a positive multiple of "
        "2 * spectrum_channel_count");
  if (!pow2(t) || t > kFilterbankMaxTscrunch)
    throw std::runtime_error(
        "pol combiner: tscrunch must be a power of two <= " +
        std::to_string(kFilterbankMaxTscrunch));
  if (f == 0 || s % f != 0)
    throw std::runtime_error(
        "pol combiner: fscrunch must divide spectrum_channel_count");
  if (cfg.nbits != 8 && cfg.nbits != 32)
    throw std::runtime_error("pol combiner: nbits must be 8 or 32");
  p_ = pol_state_nifs(cfg.pol_state);
  if (p_ == 0)
    throw std::runtime_error(
        "pol combiner: pol_state must be I (0), AABBCRCI (1) or IQUV (2)");
  l_ = n / 2 / s;
  if (l_ % 2 != 0)
    throw std::runtime_error(
        "pol combiner: baseband_input_count / spectrum_channel_count must "
        "give at least 2 time samples per channel");
  if (cfg.nsamps_reserved >= n || (n - cfg.nsamps_reserved) % (2 * s * t) != 0)
    throw std::runtime_error(
        "pol combiner: baseband_input_count - nsamps_reserved must be a "
        "positive multiple of 2 * spectrum_channel_count * tscrunch = " +
        std::to_string(2 * s * t));
  v_ = (n - cfg.nsamps_reserved) / (2 * s);
  r_ = v_ / t;
  c_ = s / f;

  check_hip(hipStreamCreateWithFlags(&stream_, hipStreamNonBlocking),
            "pol combiner stream");
  const size_t cells = r_ * (size_t)p_ * c_, pc = (size_t)p_ * c_;
  slots_.resize(n_slots);
  for (Slot& s : slots_) {
    check_hip(hipMalloc(&s.power, cells * sizeof(float)), "pol power alloc");
    if (cfg.nbits == 8) {
      check_hip(hipMalloc(&s.stats, 2 * pc * sizeof(float)), "pol stats alloc");
      check_hip(hipMalloc(&s.u8, cells), "pol u8 alloc");
      check_hip(hipMalloc(&s.partials,
                          filterbank_stats_partials(pc) * sizeof(double)),
                "pol partials alloc");
      check_hip(hipHostMalloc(&s.h_stats, 2 * pc * sizeof(float)),
                "pinned pol stats");
      check_hip(hipHostMalloc(&s.h_plane, cells), "pinned pol plane");
    } else {
      check_hip(hipHostMalloc(&s.h_plane, cells * sizeof(float)),
                "pinned pol plane");
    }
    for (hipEvent_t* e : {&s.ready_a, &s.ready_b, &s.done})
      check_hip(hipEventCreateWithFlags(e, hipEventDisableTiming),
                "pol combiner event");
  }
}

PolCombiner::~PolCombiner() {
  if (stream_) (void)hipStreamSynchronize(stream_);
  for (Slot& s : slots_) {
    if (s.power) (void)hipFree(s.power);
    if (s.stats) (void)hipFree(s.stats);
    if (s.u8) (void)hipFree(s.u8);
    if (s.partials) (void)hipFree(s.partials);
    if (s.h_plane) (void)hipHostFree(s.h_plane);
    if (s.h_stats) (void)hipHostFree(s.h_stats);
    for (hipEvent_t e : {s.ready_a, s.ready_b, s.done})
      if (e) (void)hipEventDestroy(e);
  }
  if (stream_) (void)hipStreamDestroy(stream_);
}

int PolCombiner::submit(PipelineEngine& a, int slot_a, PipelineEngine& b,
                        int slot_b) {
  auto differs = [&](const char* what, size_t va, size_t vb, size_t mine) {
    if (va != vb || va != mine)
      throw std::runtime_error(
          std::string("pol combiner: ") + what + " differs (engine a " +
          std::to_string(va) + ", engine b " + std::to_string(vb) +
          ", combiner " + std::to_string(mine) + ")");
  };
  differs("baseband_input_count", a.n(), b.n(), cfg_.baseband_input_count);
  differs("spectrum_channel_count", a.n_channels(), b.n_channels(),
          cfg_.spectrum_channel_count);
  differs("waterfall length", a.waterfall_len(), b.waterfall_len(), l_);

  const int k = next_slot_;
  next_slot_ = (next_slot_ + 1) % (int)slots_.size();
  Slot& s = slots_[k];
  if (s.busy) wait(k);

  check_hip(hipEventRecord(s.ready_a, a.stream(slot_a)), "pol ready a");
  check_hip(hipEventRecord(s.ready_b, b.stream(slot_b)), "pol ready b");
  check_hip(hipStreamWaitEvent(stream_, s.ready_a, 0), "pol wait a");
  check_hip(hipStreamWaitEvent(stream_, s.ready_b, 0), "pol wait b");
  check_hip(filterbank_detect_pol(
                a.waterfall_unzapped_ptr(slot_a),
                b.waterfall_unzapped_ptr(slot_b), a.sk_flags_ptr(slot_a),
                b.sk_flags_ptr(slot_b), cfg_.spectrum_channel_count, l_, v_,
                cfg_.tscrunch, cfg_.fscrunch, cfg_.reverse, cfg_.pol_state,
                s.power, stream_),
            "pol detect");
  const size_t pc = (size_t)p_ * c_, cells = r_ * pc;
  if (cfg_.nbits == 8) {
    // the [R][P][C] plane is the [R][P*C] plane of the per-channel kernels
    float* mean = s.stats;
    float* stddev = s.stats + pc;
    check_hip(filterbank_channel_stats(s.power, r_, pc, s.partials, mean,
                                       stddev, stream_),
              "pol stats");
    check_hip(filterbank_quantize(s.power, mean, stddev, r_, pc, s.u8,
                                  stream_),
              "pol quantize");
    check_hip(hipMemcpyAsync(s.h_plane, s.u8, cells, hipMemcpyDeviceToHost,
                             stream_),
              "pol d2h");
    check_hip(hipMemcpyAsync(s.h_stats, s.stats, 2 * pc * sizeof(float),
                             hipMemcpyDeviceToHost, stream_),
              "pol stats d2h");
  } else {
    check_hip(hipMemcpyAsync(s.h_plane, s.power, cells * sizeof(float),
                             hipMemcpyDeviceToHost, stream_),
              "pol d2h");
  }
  check_hip(hipEventRecord(s.done, stream_), "pol done");
  s.busy = true;
  return k;
}

void PolCombiner::wait(int k) {
  Slot& s = slots_.at(k);
  check_hip(hipEventSynchronize(s.done), "pol wait");
  s.busy = false;
}

const void* PolCombiner::host(int k) const { return slots_.at(k).h_plane; }
float* PolCombiner::power_ptr(int k) const { return slots_.at(k).power; }

const float* PolCombiner::mean_host(int k) const {
  const Slot& s = slots_.at(k);
  if (!s.h_stats)
    throw std::runtime_error("pol combiner: statistics exist only at 8 bits");
  return s.h_stats;
}

const float* PolCombiner::std_host(int k) const {
  return mean_host(k) + (size_t)p_ * c_;
}

}  // namespace srtb_hip
