// IncoherentSearch implementation (see incoherent_search.h).

#include "incoherent_search.h"

#include <algorithm>
#include <cmath>
#include <stdexcept>
#include <string>

#include "../kernels/common.h"

namespace srtb_hip {

std::vector<int32_t> incoherent_delays(double fch1, double foff, size_t C,
                                       double tsamp,
                                       const std::vector<double>& offsets) {
// every operation rounds on its own, as in srtb_amd.ref.incoherent_delays
#pragma clang fp contract(off)
  if (C == 0 || !(tsamp > 0) || !std::isfinite(fch1) || !std::isfinite(foff))
    throw std::runtime_error(
        "incoherent search: needs channels >= 1, tsamp > 0 and finite "
        "fch1 / foff");
  std::vector<double> inv2(C);
  for (size_t c = 0; c < C; ++c) {
    const double f = fch1 + (double)c * foff;
    if (!(f > 0))
      throw std::runtime_error(
          "incoherent search: every channel centre must be > 0 MHz");
    inv2[c] = 1.0 / (f * f);
  }
  std::vector<int32_t> d(offsets.size() * C);
  for (size_t t = 0; t < offsets.size(); ++t) {
    const double delta = offsets[t];
    if (!std::isfinite(delta))
      throw std::runtime_error("incoherent search: offsets must be finite");
    const double k = kDispersionConstantMHz * std::fabs(delta);
    for (size_t c = 0; c < C; ++c) {
      const double diff =
          delta >= 0 ? inv2[c] - inv2[0] : inv2[C - 1] - inv2[c];
      const double rows = std::nearbyint(k * diff / tsamp);
      // foff > 0 would make these negative; the limit check rejects both
      if (!(rows >= 0) || rows > (double)kIncohMaxDelay)
        throw std::runtime_error(
            "incoherent search: a delay of " + std::to_string(rows) +
            " rows is outside 0 .. " + std::to_string(kIncohMaxDelay) +
            " (offset " + std::to_string(delta) + ")");
      d[t * C + c] = (int32_t)rows;
    }
  }
  return d;
}

IncoherentSearch::IncoherentSearch(const IncoherentSearchConfig& cfg,
                                   int n_slots)
    : cfg_(cfg) {
  const size_t T = cfg.offsets.size(), R = cfg.rows, C = cfg.channels;
  if (n_slots < 1)
    throw std::runtime_error("incoherent search: n_slots must be >= 1");
  if (T < 1 || T > kIncohMaxTrials)
    throw std::runtime_error("incoherent search: needs 1 .. " +
                             std::to_string(kIncohMaxTrials) + " offsets");
  if (R < kIncohMinRows || R > kIncohMaxRows)
    throw std::runtime_error("incoherent search: rows per block must be " +
                             std::to_string(kIncohMinRows) + " .. " +
                             std::to_string(kIncohMaxRows));
  if (C < 1) throw std::runtime_error("incoherent search: needs channels >= 1");
  if (cfg.max_boxcar < 1)
    throw std::runtime_error("incoherent search: max_boxcar must be >= 1");
  if (cfg.normalize_blocks < 1 || cfg.normalize_blocks > kIncohNormMaxBlocks)
    throw std::runtime_error("incoherent search: normalize_blocks must be "
                             "1 .. " + std::to_string(kIncohNormMaxBlocks));
  nl_ = incoh_lengths(cfg.max_boxcar);
  delays_ = incoherent_delays(cfg.fch1, cfg.foff, C, cfg.tsamp, cfg.offsets);
  for (int32_t d : delays_)
    if ((size_t)d > d_max_) d_max_ = (size_t)d;
  ring_rows_ = d_max_ + R;
  if (ring_rows_ * C * sizeof(float) > kIncohMaxWindowBytes)
    throw std::runtime_error(
        "incoherent search: the history of (D_max + R) * C * 4 = " +
        std::to_string(ring_rows_ * C * sizeof(float)) + " bytes (D_max = " +
        std::to_string(d_max_) + " rows) exceeds the cap of " +
        std::to_string(kIncohMaxWindowBytes));

  check_hip(hipStreamCreateWithFlags(&stream_, hipStreamNonBlocking),
            "incoherent stream");
  check_hip(hipMalloc(&ring_, ring_rows_ * C * sizeof(float)),
            "incoherent ring alloc");
  check_hip(hipMalloc(&d_delays_, delays_.size() * sizeof(int)),
            "incoherent delays alloc");
  check_hip(hipMemcpy(d_delays_, delays_.data(), delays_.size() * sizeof(int),
                      hipMemcpyHostToDevice),
            "incoherent delays h2d");
  if (const size_t np = incoh_partials(T, R, C))
    check_hip(hipMalloc(&partials_, np * sizeof(float)),
              "incoherent partials alloc");
  if (cfg.normalize) {
    check_hip(hipMalloc(&norm_m_, 2 * C * sizeof(double)),
              "incoherent normalisation alloc");
    norm_v_ = norm_m_ + C;
    check_hip(hipMalloc(&norm_g_, C * sizeof(float)),
              "incoherent normalisation alloc");
    check_hip(hipMalloc(&norm_partials_,
                        incoh_norm_partials(C) * sizeof(double)),
              "incoherent normalisation alloc");
  }
  const size_t tl = T * (size_t)nl_;
  const size_t n_u32 = 2 * tl + (cfg.normalize ? 1 : 0);
  slots_.resize(n_slots);
  for (Slot& s : slots_) {
    check_hip(hipMalloc(&s.y, T * R * sizeof(float)), "incoherent plane alloc");
    check_hip(hipMalloc(&s.res_f64, (2 * tl + T) * sizeof(double)),
              "incoherent result alloc");
    check_hip(hipMalloc(&s.res_u32, n_u32 * sizeof(unsigned)),
              "incoherent result alloc");
    check_hip(hipHostMalloc(&s.h_y, T * R * sizeof(float)),
              "pinned incoherent plane");
    check_hip(hipHostMalloc(&s.h_f64, (2 * tl + T) * sizeof(double)),
              "pinned incoherent result");
    check_hip(hipHostMalloc(&s.h_u32, n_u32 * sizeof(unsigned)),
              "pinned incoherent result");
    for (hipEvent_t* e : {&s.ready, &s.done})
      check_hip(hipEventCreateWithFlags(e, hipEventDisableTiming),
                "incoherent event");
  }
  reset();
}

IncoherentSearch::~IncoherentSearch() {
  if (stream_) (void)hipStreamSynchronize(stream_);
  for (Slot& s : slots_) {
    if (s.y) (void)hipFree(s.y);
    if (s.res_f64) (void)hipFree(s.res_f64);
    if (s.res_u32) (void)hipFree(s.res_u32);
    if (s.h_y) (void)hipHostFree(s.h_y);
    if (s.h_f64) (void)hipHostFree(s.h_f64);
    if (s.h_u32) (void)hipHostFree(s.h_u32);
    for (hipEvent_t e : {s.ready, s.done})
      if (e) (void)hipEventDestroy(e);
  }
  if (ring_) (void)hipFree(ring_);
  if (d_delays_) (void)hipFree(d_delays_);
  if (partials_) (void)hipFree(partials_);
  if (norm_m_) (void)hipFree(norm_m_);
  if (norm_g_) (void)hipFree(norm_g_);
  if (norm_partials_) (void)hipFree(norm_partials_);
  if (stream_) (void)hipStreamDestroy(stream_);
}

void IncoherentSearch::reset() {
  // stream-ordered behind every block already submitted
  check_hip(hipMemsetAsync(ring_, 0,
                           ring_rows_ * cfg_.channels * sizeof(float),
                           stream_),
            "incoherent reset");
  if (cfg_.normalize) {
    check_hip(hipMemsetAsync(norm_m_, 0, 2 * cfg_.channels * sizeof(double),
                             stream_),
              "incoherent reset");
    check_hip(hipMemsetAsync(norm_g_, 0, cfg_.channels * sizeof(float),
                             stream_),
              "incoherent reset");
  }
  write_row_ = 0;
  block_ = 0;
}

int IncoherentSearch::submit(PipelineEngine& eng, int slot) {
  if (eng.filterbank_rows() != cfg_.rows ||
      eng.filterbank_channels() != cfg_.channels)
    throw std::runtime_error(
        "incoherent search: the engine's filterbank plane is " +
        std::to_string(eng.filterbank_rows()) + " x " +
        std::to_string(eng.filterbank_channels()) + ", the searcher's " +
        std::to_string(cfg_.rows) + " x " + std::to_string(cfg_.channels));
  const float* plane = eng.filterbank_power_ptr(slot);
  Slot& s = slots_[next_slot_];
  if (s.busy) wait(next_slot_);
  check_hip(hipEventRecord(s.ready, eng.stream(slot)), "incoherent ready");
  return submit_plane(plane, s.ready);
}

int IncoherentSearch::submit_plane(const float* dev_plane, hipEvent_t ready) {
  if (!dev_plane) throw std::runtime_error("incoherent search: null plane");
  const int k = next_slot_;
  next_slot_ = (next_slot_ + 1) % (int)slots_.size();
  Slot& s = slots_[k];
  if (s.busy) wait(k);
  const size_t T = cfg_.offsets.size(), R = cfg_.rows, C = cfg_.channels;

  if (ready) check_hip(hipStreamWaitEvent(stream_, ready, 0), "incoherent wait");
  const size_t tl = T * (size_t)nl_;
  // the block's R rows go to ring rows write_row_ ..., wrapping at most once
  if (cfg_.normalize) {
    // the state that normalises block b includes block b
    const uint64_t seen = block_ + 1;
    const double alpha =
        1.0 / (double)std::min<uint64_t>(seen, cfg_.normalize_blocks);
    check_hip(incoh_norm_update(dev_plane, R, C, alpha, norm_partials_,
                                norm_m_, norm_v_, norm_g_, s.res_u32 + 2 * tl,
                                stream_),
              "incoherent normalisation");
    check_hip(incoh_norm_apply(dev_plane, R, C, norm_m_, norm_g_, ring_,
                               ring_rows_, write_row_, stream_),
              "incoherent normalisation");
  } else {
    const size_t first = std::min(R, ring_rows_ - write_row_);
    check_hip(hipMemcpyAsync(ring_ + write_row_ * C, dev_plane,
                             first * C * sizeof(float),
                             hipMemcpyDeviceToDevice, stream_),
              "incoherent history");
    if (first < R)
      check_hip(hipMemcpyAsync(ring_, dev_plane + first * C,
                               (R - first) * C * sizeof(float),
                               hipMemcpyDeviceToDevice, stream_),
                "incoherent history");
  }
  write_row_ = (write_row_ + R) % ring_rows_;
  // the ring holds exactly D_max + R rows: the oldest, global row
  // block * R - D_max, follows the newest
  check_hip(incoh_dedisperse(ring_, ring_rows_, write_row_, d_delays_, T, R, C,
                             partials_, s.y, stream_),
            "incoherent dedisperse");
  s.block = block_;
  s.valid = block_ * R >= d_max_;
  s.first_row = (int64_t)(block_ * R) - (int64_t)d_max_;
  ++block_;
  if (s.valid) {
    check_hip(incoh_detect(s.y, T, R, nl_, cfg_.snr_threshold, s.res_f64,
                           s.res_u32, s.res_f64 + tl, s.res_u32 + tl,
                           s.res_f64 + 2 * tl, stream_),
              "incoherent detect");
    check_hip(hipMemcpyAsync(s.h_f64, s.res_f64, (2 * tl + T) * sizeof(double),
                             hipMemcpyDeviceToHost, stream_),
              "incoherent result d2h");
    // with normalize, the live count rides behind the counts
    check_hip(hipMemcpyAsync(s.h_u32, s.res_u32,
                             (2 * tl + (cfg_.normalize ? 1 : 0)) *
                                 sizeof(unsigned),
                             hipMemcpyDeviceToHost, stream_),
              "incoherent result d2h");
  } else if (cfg_.normalize) {
    check_hip(hipMemcpyAsync(s.h_u32 + 2 * tl, s.res_u32 + 2 * tl,
                             sizeof(unsigned), hipMemcpyDeviceToHost, stream_),
              "incoherent result d2h");
  }
  check_hip(hipMemcpyAsync(s.h_y, s.y, T * R * sizeof(float),
                           hipMemcpyDeviceToHost, stream_),
            "incoherent plane d2h");
  check_hip(hipEventRecord(s.done, stream_), "incoherent done");
  s.busy = true;
  return k;
}

IncoherentResult IncoherentSearch::wait(int k) {
  Slot& s = slots_.at(k);
  check_hip(hipEventSynchronize(s.done), "incoherent wait");
  s.busy = false;
  IncoherentResult r;
  r.valid = s.valid;
  r.first_row = s.first_row;
  r.block = s.block;
  const size_t T = cfg_.offsets.size(), tl = T * (size_t)nl_;
  if (cfg_.normalize) r.live_channels = s.h_u32[2 * tl];
  if (!s.valid) return r;
  r.trials.resize(T);
  for (size_t t = 0; t < T; ++t) {
    IncoherentTrial& tr = r.trials[t];
    tr.offset = cfg_.offsets[t];
    tr.mean = s.h_f64[2 * tl + t];
    tr.lengths.resize(nl_);
    for (int l = 0; l < nl_; ++l) {
      IncoherentDetection& d = tr.lengths[l];
      const size_t o = t * (size_t)nl_ + l;
      d.boxcar_length = (size_t)1 << l;
      d.peak = s.h_f64[o];
      d.rms = s.h_f64[tl + o];
      d.index = s.h_u32[o];
      d.count = s.h_u32[tl + o];
      d.snr = d.rms > 0 ? d.peak / d.rms : 0.0;
    }
  }
  return r;
}

float* IncoherentSearch::plane_ptr(int k) const { return slots_.at(k).y; }
const float* IncoherentSearch::plane_host(int k) const {
  return slots_.at(k).h_y;
}

}  // namespace srtb_hip
