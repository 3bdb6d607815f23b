// Torch-extension bindings for srtb_amd: granular kernel ops (for numerics
// tests and composition) + the native PipelineEngine.
//
// The kernels themselves live in csrc/kernels/*.hip (pure HIP, no torch);
// this TU only adapts torch::Tensor ↔ raw pointers and streams.

#include <torch/extension.h>
#include <pybind11/numpy.h>
#include <ATen/cuda/CUDAContext.h>
#include <c10/cuda/CUDAGuard.h>

#include <functional>
#include <vector>

#include "../engine/engine.h"
#include "../engine/incoherent_search.h"
#include "../engine/pol_combiner.h"
#include "../fft/native_fft.h"
#include "../include/srtb_kernels.h"

namespace {

using namespace srtb_hip;

hipStream_t cur_stream() {
  return at::cuda::getCurrentCUDAStream().stream();
}

void check(hipError_t e, const char* what) { check_hip(e, what); }

#define CHECK_CUDA(t) TORCH_CHECK((t).is_cuda(), #t " must be on GPU")
#define CHECK_CONTIG(t) TORCH_CHECK((t).is_contiguous(), #t " must be contiguous")

// the float32 window of at least `count` coefficients, or null
const float* window_ptr(const c10::optional<torch::Tensor>& window,
                        size_t count) {
  if (!window.has_value()) return nullptr;
  CHECK_CUDA(*window);
  CHECK_CONTIG(*window);
  TORCH_CHECK(window->scalar_type() == torch::kFloat32 &&
                  (size_t)window->numel() >= count,
              "window must be float32 with at least ", count, " coefficients");
  return window->data_ptr<float>();
}

float2* cptr(torch::Tensor& t) {
  return reinterpret_cast<float2*>(t.data_ptr());
}
const float2* cptr(const torch::Tensor& t) {
  return reinterpret_cast<const float2*>(t.data_ptr());
}

torch::Tensor t_unpack(torch::Tensor raw, int64_t nbits, int64_t out_count,
                       c10::optional<torch::Tensor> window) {
  CHECK_CUDA(raw);
  CHECK_CONTIG(raw);
  TORCH_CHECK(raw.scalar_type() == torch::kUInt8 && out_count >= 0);
  const size_t need_bits = (size_t)out_count * (size_t)std::abs(nbits);
  TORCH_CHECK((size_t)raw.numel() * 8 >= need_bits, "unpack: ", out_count,
              " samples of ", nbits, " bits need more than the ", raw.numel(),
              " bytes given");
  auto out = torch::empty({out_count},
                          raw.options().dtype(torch::kFloat32));
  const float* w = window_ptr(window, (size_t)out_count);
  check(unpack(raw.data_ptr<uint8_t>(), out.data_ptr<float>(), out_count,
               (int)nbits, w, cur_stream()),
        "unpack");
  return out;
}

std::vector<torch::Tensor> t_unpack_2pol(torch::Tensor raw, std::string kind,
                                         c10::optional<torch::Tensor> window) {
  CHECK_CUDA(raw);
  CHECK_CONTIG(raw);
  TORCH_CHECK(raw.element_size() == 1 && raw.numel() % 2 == 0,
              "unpack_2pol: raw must be an even number of bytes");
  const size_t per_pol = raw.numel() / 2;
  const float* w = window_ptr(window, per_pol);
  auto o0 = torch::empty({(int64_t)per_pol}, raw.options().dtype(torch::kFloat32));
  auto o1 = torch::empty({(int64_t)per_pol}, raw.options().dtype(torch::kFloat32));
  auto* p = reinterpret_cast<const int8_t*>(raw.data_ptr());
  if (kind == "interleave")
    check(unpack_interleaved_2pol(p, o0.data_ptr<float>(), o1.data_ptr<float>(),
                                  per_pol, w, cur_stream()),
          "unpack_2pol");
  else if (kind == "naocpsr_snap1")
    check(unpack_naocpsr_snap1(p, o0.data_ptr<float>(), o1.data_ptr<float>(),
                               per_pol, w, cur_stream()),
          "unpack_snap1");
  else
    TORCH_CHECK(false, "unknown 2-pol kind ", kind);
  return {o0, o1};
}

std::vector<torch::Tensor> t_unpack_gznupsr(
    torch::Tensor raw, int64_t n_streams,
    c10::optional<torch::Tensor> window) {
  CHECK_CUDA(raw);
  CHECK_CONTIG(raw);
  TORCH_CHECK(n_streams == 2 || n_streams == 4,
              "unpack_gznupsr_a1: 2 or 4 streams");
  TORCH_CHECK(raw.element_size() == 1 && raw.numel() % n_streams == 0,
              "unpack_gznupsr_a1: raw must be a whole number of bytes per "
              "stream");
  const size_t per = raw.numel() / n_streams;
  const float* w = window_ptr(window, per);
  std::vector<torch::Tensor> outs;
  float* ptrs[4] = {nullptr, nullptr, nullptr, nullptr};
  for (int i = 0; i < n_streams; ++i) {
    outs.push_back(torch::empty({(int64_t)per},
                                raw.options().dtype(torch::kFloat32)));
    ptrs[i] = outs.back().data_ptr<float>();
  }
  check(unpack_gznupsr_a1(raw.data_ptr<uint8_t>(), ptrs[0], ptrs[1], ptrs[2],
                          ptrs[3], (int)n_streams, per, w, cur_stream()),
        "unpack_gznupsr");
  return outs;
}

// the engine's window table (0 = rectangle, 1 = hann, 2 = hamming)
torch::Tensor t_build_window(int64_t n, int64_t kind, torch::Device dev) {
  TORCH_CHECK(n >= 0, "build_window: n must not be negative");
  auto out = torch::empty({n}, torch::TensorOptions()
                                   .dtype(torch::kFloat32)
                                   .device(dev));
  check(build_window(out.data_ptr<float>(), (size_t)n, (int)kind,
                     cur_stream()),
        "build_window");
  return out;
}

// blocks (optional): the pass-1 grid, a test surface for the fp64 drain
torch::Tensor t_mean_power(torch::Tensor spec, int64_t blocks = 0) {
  CHECK_CUDA(spec);
  CHECK_CONTIG(spec);
  TORCH_CHECK(spec.scalar_type() == torch::kComplexFloat);
  TORCH_CHECK(blocks >= 0 && blocks <= reduce_partials() / 2,
              "mean_power: blocks must be 0 (default) or 1 .. ",
              reduce_partials() / 2);
  auto partials = torch::empty({reduce_partials()},
                               spec.options().dtype(torch::kFloat64));
  auto out = torch::empty({1}, spec.options().dtype(torch::kFloat64));
  check(mean_power(cptr(spec), spec.numel(),
                   partials.data_ptr<double>(), out.data_ptr<double>(),
                   cur_stream(), (int)blocks),
        "mean_power");
  return out;
}

torch::Tensor t_sum_sumsq(torch::Tensor x) {
  CHECK_CUDA(x);
  CHECK_CONTIG(x);
  auto partials = torch::empty({reduce_partials()},
                               x.options().dtype(torch::kFloat64));
  auto out = torch::empty({2}, x.options().dtype(torch::kFloat64));
  check(sum_sumsq(x.data_ptr<float>(), x.numel(), partials.data_ptr<double>(),
                  out.data_ptr<double>(), cur_stream()),
        "sum_sumsq");
  return out;
}

void t_rfi_s1(torch::Tensor spec, double threshold, int64_t channel_count) {
  CHECK_CUDA(spec);
  CHECK_CONTIG(spec);
  auto mean = t_mean_power(spec);
  const size_t n = spec.numel();
  const float coeff =
      (float)std::pow((double)n * (double)n / (double)channel_count, -0.5);
  check(rfi_s1(cptr(spec), n, mean.data_ptr<double>(), (float)threshold,
               coeff, cur_stream()),
        "rfi_s1");
}

void t_zap_bins(torch::Tensor spec, int64_t lo, int64_t hi) {
  CHECK_CUDA(spec);
  CHECK_CONTIG(spec);
  TORCH_CHECK(spec.scalar_type() == torch::kComplexFloat,
              "zap_bins: spec must be complex64");
  TORCH_CHECK(0 <= lo && lo <= hi && hi < spec.numel(),
              "zap_bins: need 0 <= lo <= hi < ", spec.numel(), ", got ", lo,
              " and ", hi);
  check(zap_bins(cptr(spec), lo, hi, cur_stream()), "zap_bins");
}

void t_dedisperse(torch::Tensor spec, double f_min, double f_c, double df,
                  double dm) {
  CHECK_CUDA(spec);
  CHECK_CONTIG(spec);
  check(dedisperse(cptr(spec), spec.numel(), f_min, f_c, df, dm, cur_stream()),
        "dedisperse");
}

torch::Tensor t_phase_table(int64_t n, double f_min, double f_c, double df,
                            double dm, torch::Device dev) {
  auto out = torch::empty({n}, torch::TensorOptions()
                                   .dtype(torch::kComplexFloat)
                                   .device(dev));
  check(dedisp_phase_table(cptr(out), n, f_min, f_c, df, dm, cur_stream()),
        "phase_table");
  return out;
}

void t_rfi_dedisperse_fused(torch::Tensor spec, bool enable_rfi,
                            double threshold, int64_t channel_count,
                            std::vector<std::vector<int64_t>> ranges,
                            double f_min, double f_c, double df, double dm,
                            c10::optional<torch::Tensor> table,
                            c10::optional<torch::Tensor> out) {
  CHECK_CUDA(spec);
  CHECK_CONTIG(spec);
  const size_t n = spec.numel();
  // out= (optional): write the result there and leave spec untouched;
  // out aliasing spec is the in-place call
  float2* dst = cptr(spec);
  if (out.has_value()) {
    CHECK_CUDA(*out);
    CHECK_CONTIG(*out);
    TORCH_CHECK(out->scalar_type() == spec.scalar_type() &&
                    (size_t)out->numel() == n,
                "out must match spec in dtype and size");
    dst = cptr(*out);
  }
  torch::Tensor mean;
  const double* mp = nullptr;
  if (enable_rfi) {
    mean = t_mean_power(spec);
    mp = mean.data_ptr<double>();
  }
  const float coeff =
      (float)std::pow((double)n * (double)n / (double)channel_count, -0.5);
  ZapRange zr[16];
  TORCH_CHECK(ranges.size() <= 16, "at most 16 zap ranges");
  for (size_t i = 0; i < ranges.size(); ++i) {
    zr[i].lo = (unsigned long long)ranges[i][0];
    zr[i].hi = (unsigned long long)ranges[i][1];
  }
  const float2* tb = nullptr;
  if (table.has_value()) {
    CHECK_CUDA(*table);
    CHECK_CONTIG(*table);
    TORCH_CHECK(table->scalar_type() == torch::kComplexFloat &&
                    (size_t)table->numel() >= n,
                "table must be complex64 with at least ", n, " factors");
    tb = cptr(*table);
  }
  check(rfi_dedisperse_fused(static_cast<const float2*>(cptr(spec)), dst, n,
                             mp, (float)threshold, coeff, zr,
                             (int)ranges.size(), f_min, f_c, df, dm, tb,
                             cur_stream()),
        "rfi_dedisperse_fused");
}

// (values, indices) of the raw-series peak and of every boxcar length's
std::vector<torch::Tensor> t_detect_peaks(torch::Tensor ts,
                                          torch::Tensor cumsum,
                                          std::vector<int64_t> lengths) {
  CHECK_CUDA(ts);
  CHECK_CONTIG(ts);
  CHECK_CUDA(cumsum);
  CHECK_CONTIG(cumsum);
  TORCH_CHECK(ts.scalar_type() == torch::kFloat32 &&
              cumsum.scalar_type() == torch::kFloat32);
  TORCH_CHECK(lengths.empty() || cumsum.numel() == ts.numel(),
              "cumsum must have ts's length");
  TORCH_CHECK(lengths.size() <= 12, "at most 12 boxcar lengths");
  std::vector<size_t> ls;
  for (int64_t L : lengths) {
    TORCH_CHECK(L > 0, "boxcar lengths must be positive");
    ls.push_back((size_t)L);
  }
  const int64_t n_out = 1 + (int64_t)ls.size();
  auto scratch = torch::empty({(int64_t)detect_peaks_scratch_bytes()},
                              ts.options().dtype(torch::kUInt8));
  auto values = torch::empty({n_out}, ts.options());
  auto indices = torch::empty({n_out}, ts.options().dtype(torch::kInt32));
  check(detect_peaks(ts.data_ptr<float>(), cumsum.data_ptr<float>(),
                     ts.numel(), ls.data(), (int)ls.size(),
                     scratch.data_ptr(), values.data_ptr<float>(),
                     reinterpret_cast<unsigned*>(indices.data_ptr<int32_t>()),
                     cur_stream()),
        "detect_peaks");
  return {values, indices.to(torch::kInt64)};
}

torch::Tensor t_sk_row_stats(torch::Tensor wf) {
  CHECK_CUDA(wf);
  CHECK_CONTIG(wf);
  TORCH_CHECK(wf.dim() == 2);
  const size_t rows = wf.size(0), len = wf.size(1);
  auto out = torch::empty({(int64_t)rows, 2},
                          wf.options().dtype(torch::kFloat32));
  check(sk_row_stats(cptr(wf), rows, len,
                     reinterpret_cast<float2*>(out.data_ptr<float>()),
                     cur_stream()),
        "sk_row_stats");
  return out;
}

std::vector<torch::Tensor> t_sk_mitigate(torch::Tensor wf, double sk_threshold) {
  CHECK_CUDA(wf);
  CHECK_CONTIG(wf);
  TORCH_CHECK(wf.dim() == 2);
  const size_t rows = wf.size(0), len = wf.size(1);
  auto s2s4 = t_sk_row_stats(wf);
  double hi = sk_threshold, lo = 2.0 - hi;
  if (lo > hi) std::swap(lo, hi);
  const double corr = ((double)len - 1.0) / ((double)len + 1.0);
  auto flags = torch::empty({(int64_t)rows}, wf.options().dtype(torch::kUInt8));
  auto zero_count = torch::zeros({1}, wf.options().dtype(torch::kInt32));
  check(sk_flags(cptr(wf), reinterpret_cast<float2*>(s2s4.data_ptr<float>()),
                 rows, len, (float)(lo * corr + 1.0), (float)(hi * corr + 1.0),
                 flags.data_ptr<uint8_t>(),
                 reinterpret_cast<unsigned*>(zero_count.data_ptr<int32_t>()),
                 cur_stream()),
        "sk_flags");
  check(sk_zap_rows(cptr(wf), flags.data_ptr<uint8_t>(), rows, len,
                    cur_stream()),
        "sk_zap");
  return {flags, zero_count};
}

torch::Tensor t_sk_v1_mitigate(torch::Tensor wf, double sk_threshold,
                               bool normalize) {
  CHECK_CUDA(wf);
  CHECK_CONTIG(wf);
  TORCH_CHECK(wf.dim() == 2);  // [M][bins], time-major
  const size_t M = wf.size(0), bins = wf.size(1);
  auto s2s4 = torch::empty({(int64_t)bins, 2},
                           wf.options().dtype(torch::kFloat32));
  check(sk_v1_stats(cptr(wf), M, bins,
                    reinterpret_cast<float2*>(s2s4.data_ptr<float>()),
                    cur_stream()),
        "sk_v1_stats");
  double hi = sk_threshold, lo = 2.0 - hi;
  if (lo > hi) std::swap(lo, hi);
  const double corr = ((double)M - 1.0) / ((double)M + 1.0);
  check(sk_v1_zap(cptr(wf), M, bins,
                  reinterpret_cast<const float2*>(s2s4.data_ptr<float>()),
                  (float)(lo * corr + 1.0), (float)(hi * corr + 1.0),
                  normalize, cur_stream()),
        "sk_v1_zap");
  return s2s4;
}

torch::Tensor t_time_series(torch::Tensor wf,
                            c10::optional<torch::Tensor> flags,
                            int64_t ts_count) {
  CHECK_CUDA(wf);
  CHECK_CONTIG(wf);
  TORCH_CHECK(wf.dim() == 2);
  const size_t rows = wf.size(0), len = wf.size(1);
  auto out = torch::empty({ts_count}, wf.options().dtype(torch::kFloat32));
  const uint8_t* f = flags.has_value() ? flags->data_ptr<uint8_t>() : nullptr;
  auto scratch = torch::empty(
      {(int64_t)time_series_chunks(ts_count) * ts_count},
      wf.options().dtype(torch::kFloat32));
  check(time_series_2stage(cptr(wf), f, rows, len, ts_count,
                           out.data_ptr<float>(), scratch.data_ptr<float>(),
                           cur_stream()),
        "time_series");
  return out;
}

void t_subtract_mean(torch::Tensor ts) {
  CHECK_CUDA(ts);
  auto sums = t_sum_sumsq(ts);
  check(subtract_mean(ts.data_ptr<float>(), ts.numel(),
                      sums.data_ptr<double>(), cur_stream()),
        "subtract_mean");
}

std::vector<torch::Tensor> t_count_signal(torch::Tensor ts, double snr) {
  CHECK_CUDA(ts);
  auto sums = t_sum_sumsq(ts);
  auto count = torch::zeros({1}, ts.options().dtype(torch::kInt32));
  auto thr = torch::empty({1}, ts.options().dtype(torch::kFloat32));
  check(count_above(ts.data_ptr<float>(), ts.numel(),
                    sums.data_ptr<double>() + 1, (float)snr,
                    reinterpret_cast<unsigned*>(count.data_ptr<int32_t>()),
                    thr.data_ptr<float>(), cur_stream()),
        "count_above");
  return {count, thr};
}

torch::Tensor t_inclusive_scan(torch::Tensor ts) {
  CHECK_CUDA(ts);
  auto out = torch::empty_like(ts);
  auto scratch = torch::empty({std::max<int64_t>(4096,
                                  scan_scratch_size(ts.numel()))},
                              ts.options());
  check(inclusive_scan(ts.data_ptr<float>(), out.data_ptr<float>(),
                       ts.numel(), scratch.data_ptr<float>(), cur_stream()),
        "inclusive_scan");
  return out;
}

// (thresholds float32 [n], counts int32 [n]) of the fused boxcar ladder
std::vector<torch::Tensor> t_boxcar_ladder(torch::Tensor cumsum,
                                           std::vector<int64_t> lengths,
                                           double snr) {
  CHECK_CUDA(cumsum);
  CHECK_CONTIG(cumsum);
  TORCH_CHECK(cumsum.scalar_type() == torch::kFloat32);
  TORCH_CHECK(!lengths.empty() && lengths.size() <= 12,
              "1 to 12 boxcar lengths");
  std::vector<size_t> ls;
  for (int64_t L : lengths) {
    TORCH_CHECK(L > 0, "boxcar lengths must be positive");
    ls.push_back((size_t)L);
  }
  const int64_t nl = (int64_t)ls.size();
  auto partials = torch::empty({nl * 2 * reduce_partials()},
                               cumsum.options().dtype(torch::kFloat64));
  auto thr = torch::empty({nl}, cumsum.options());
  auto counts = torch::zeros({nl}, cumsum.options().dtype(torch::kInt32));
  check(boxcar_ladder(cumsum.data_ptr<float>(), cumsum.numel(), ls.data(),
                      (int)nl, partials.data_ptr<double>(), (float)snr,
                      thr.data_ptr<float>(),
                      reinterpret_cast<unsigned*>(counts.data_ptr<int32_t>()),
                      cur_stream()),
        "boxcar_ladder");
  return {thr, counts};
}

torch::Tensor t_boxcar(torch::Tensor cumsum, int64_t L) {
  CHECK_CUDA(cumsum);
  const int64_t n_out = cumsum.numel() - L;
  auto out = torch::empty({n_out}, cumsum.options());
  check(boxcar(cumsum.data_ptr<float>(), out.data_ptr<float>(), n_out, L,
               cur_stream()),
        "boxcar");
  return out;
}

torch::Tensor t_resample_power(torch::Tensor wf, int64_t H, int64_t W) {
  CHECK_CUDA(wf);
  CHECK_CONTIG(wf);
  TORCH_CHECK(wf.dim() == 2 && wf.scalar_type() == torch::kComplexFloat);
  TORCH_CHECK(wf.size(0) >= 1 && wf.size(1) >= 1 && H >= 1 && W >= 1 &&
                  H <= INT32_MAX && W <= INT32_MAX && H * W <= INT32_MAX,
              "resample_power: rows, len, H and W must all be >= 1");
  auto out = torch::empty({H, W}, wf.options().dtype(torch::kFloat32));
  check(resample_power_2d(cptr(wf), wf.size(0), wf.size(1),
                          out.data_ptr<float>(), (int)H, (int)W, cur_stream()),
        "resample");
  return out;
}

void t_normalize_by_mean(torch::Tensor img) {
  CHECK_CUDA(img);
  auto sums = t_sum_sumsq(img);
  check(normalize_by_mean(img.data_ptr<float>(), img.numel(),
                          sums.data_ptr<double>(), cur_stream()),
        "normalize");
}

torch::Tensor t_generate_pixmap(torch::Tensor img, int64_t c0, int64_t c1,
                                int64_t cover) {
  CHECK_CUDA(img);
  CHECK_CONTIG(img);
  TORCH_CHECK(img.scalar_type() == torch::kFloat32,
              "generate_pixmap: img must be float32");
  auto out = torch::empty_like(img, img.options().dtype(torch::kInt32));
  check(generate_pixmap(img.data_ptr<float>(),
                        reinterpret_cast<uint32_t*>(out.data_ptr<int32_t>()),
                        img.numel(), (uint32_t)c0, (uint32_t)c1,
                        (uint32_t)cover, cur_stream()),
        "pixmap");
  return out;
}

std::vector<torch::Tensor> t_running_mean(torch::Tensor data,
                                          int64_t windowsize) {
  CHECK_CUDA(data);
  CHECK_CONTIG(data);
  TORCH_CHECK(data.dim() == 2 && data.scalar_type() == torch::kFloat32);
  TORCH_CHECK(windowsize >= 1 && windowsize <= data.size(0),
              "running_mean: need 1 <= windowsize <= nsamp = ", data.size(0),
              ", got ", windowsize);
  const size_t nsamp = data.size(0), nchan = data.size(1);
  auto ave = torch::empty({(int64_t)nchan}, data.options());
  auto out = torch::empty({(int64_t)nsamp, (int64_t)nchan},
                          data.options().dtype(torch::kUInt8));
  check(running_mean_init(data.data_ptr<float>(), nsamp, nchan, windowsize,
                          ave.data_ptr<float>(), cur_stream()),
        "rm init");
  check(running_mean(data.data_ptr<float>(), nsamp, nchan,
                     out.data_ptr<uint8_t>(), windowsize,
                     ave.data_ptr<float>(), cur_stream()),
        "rm");
  return {out, ave};
}

// out (optional): receives corr; it may be f1 or f2 itself
std::vector<torch::Tensor> t_correlate(torch::Tensor f1, torch::Tensor f2,
                                       double scale,
                                       c10::optional<torch::Tensor> out) {
  CHECK_CUDA(f1);
  CHECK_CUDA(f2);
  CHECK_CONTIG(f1);
  CHECK_CONTIG(f2);
  TORCH_CHECK(f1.scalar_type() == torch::kComplexFloat &&
                  f2.scalar_type() == torch::kComplexFloat,
              "correlate: f1 and f2 must be complex64");
  TORCH_CHECK(f2.numel() == f1.numel(), "correlate: f2 has ", f2.numel(),
              " elements, f1 has ", f1.numel());
  torch::Tensor corr;
  if (out.has_value()) {
    CHECK_CUDA(*out);
    CHECK_CONTIG(*out);
    TORCH_CHECK(out->scalar_type() == torch::kComplexFloat &&
                    out->numel() == f1.numel(),
                "correlate: out must match f1 in dtype and size");
    // exactly aliased or disjoint: a partial overlap would race
    for (const torch::Tensor* in : {&f1, &f2}) {
      const char* a = static_cast<const char*>(in->data_ptr());
      const char* b = static_cast<const char*>(out->data_ptr());
      const size_t bytes = (size_t)f1.numel() * sizeof(float2);
      TORCH_CHECK(a == b || a + bytes <= b || b + bytes <= a,
                  "correlate: out may alias an input only exactly");
    }
    corr = *out;
  } else {
    corr = torch::empty_like(f1);
  }
  auto mag = torch::empty({f1.numel()}, f1.options().dtype(torch::kFloat32));
  check(correlate_pointwise(cptr(f1), cptr(f2), cptr(corr),
                            mag.data_ptr<float>(), f1.numel(), (float)scale,
                            cur_stream()),
        "correlate");
  return {corr, mag};
}

torch::Tensor t_complex_abs(torch::Tensor x) {
  CHECK_CUDA(x);
  CHECK_CONTIG(x);
  TORCH_CHECK(x.scalar_type() == torch::kComplexFloat,
              "complex_abs: x must be complex64");
  auto mag = torch::empty({x.numel()}, x.options().dtype(torch::kFloat32));
  check(complex_abs(cptr(x), mag.data_ptr<float>(), x.numel(), cur_stream()),
        "complex_abs");
  return mag;
}

// ---------------- filterbank output ----------------

torch::Tensor t_filterbank_detect(torch::Tensor wf,
                                  c10::optional<torch::Tensor> flags,
                                  int64_t valid_rows, int64_t tscrunch,
                                  int64_t fscrunch, bool reverse) {
  CHECK_CUDA(wf);
  CHECK_CONTIG(wf);
  TORCH_CHECK(wf.dim() == 2 && wf.scalar_type() == torch::kComplexFloat);
  const int64_t S = wf.size(0), L = wf.size(1);
  TORCH_CHECK(tscrunch >= 1 && fscrunch >= 1 && S % fscrunch == 0 &&
                  valid_rows >= tscrunch && valid_rows <= L && L % 2 == 0,
              "filterbank_detect: bad geometry");
  const uint8_t* f = nullptr;
  if (flags.has_value()) {
    CHECK_CUDA(*flags);
    CHECK_CONTIG(*flags);
    TORCH_CHECK(flags->scalar_type() == torch::kUInt8 && flags->numel() == S);
    f = flags->data_ptr<uint8_t>();
  }
  auto out = torch::empty({valid_rows / tscrunch, S / fscrunch},
                          wf.options().dtype(torch::kFloat32));
  check(filterbank_detect(cptr(wf), f, S, L, valid_rows, tscrunch, fscrunch,
                          reverse, out.data_ptr<float>(), cur_stream()),
        "filterbank_detect");
  return out;
}

// [R][P][C] float32 polarization products of two waterfalls of the same sky
torch::Tensor t_filterbank_detect_pol(torch::Tensor wf_a, torch::Tensor wf_b,
                                      c10::optional<torch::Tensor> flags_a,
                                      c10::optional<torch::Tensor> flags_b,
                                      int64_t valid_rows, int64_t tscrunch,
                                      int64_t fscrunch, bool reverse,
                                      int64_t pol_state) {
  CHECK_CUDA(wf_a);
  CHECK_CONTIG(wf_a);
  CHECK_CUDA(wf_b);
  CHECK_CONTIG(wf_b);
  TORCH_CHECK(wf_a.dim() == 2 && wf_a.scalar_type() == torch::kComplexFloat &&
                  wf_b.dim() == 2 && wf_b.scalar_type() == torch::kComplexFloat,
              "filterbank_detect_pol: waterfalls must be 2-D complex64");
  TORCH_CHECK(wf_a.sizes() == wf_b.sizes(),
              "filterbank_detect_pol: the two waterfalls differ in shape");
  const int64_t S = wf_a.size(0), L = wf_a.size(1);
  const int P = pol_state_nifs((int)pol_state);
  TORCH_CHECK(pol_state >= 0 && P > 0,
              "filterbank_detect_pol: pol_state must be 0 (I), 1 (AABBCRCI) "
              "or 2 (IQUV)");
  TORCH_CHECK(tscrunch >= 1 && fscrunch >= 1 && S % fscrunch == 0 &&
                  valid_rows >= tscrunch && valid_rows <= L && L % 2 == 0,
              "filterbank_detect_pol: bad geometry");
  auto flag_ptr = [&](const c10::optional<torch::Tensor>& flags) {
    const uint8_t* f = nullptr;
    if (flags.has_value()) {
      CHECK_CUDA(*flags);
      CHECK_CONTIG(*flags);
      TORCH_CHECK(flags->scalar_type() == torch::kUInt8 &&
                  flags->numel() == S);
      f = flags->data_ptr<uint8_t>();
    }
    return f;
  };
  const uint8_t* fa = flag_ptr(flags_a);
  const uint8_t* fb = flag_ptr(flags_b);
  auto out = torch::empty({valid_rows / tscrunch, (int64_t)P, S / fscrunch},
                          wf_a.options().dtype(torch::kFloat32));
  check(filterbank_detect_pol(cptr(wf_a), cptr(wf_b), fa, fb, S, L, valid_rows,
                              tscrunch, fscrunch, reverse, (int)pol_state,
                              out.data_ptr<float>(), cur_stream()),
        "filterbank_detect_pol");
  return out;
}

std::vector<torch::Tensor> t_filterbank_channel_stats(torch::Tensor P) {
  CHECK_CUDA(P);
  CHECK_CONTIG(P);
  TORCH_CHECK(P.dim() == 2 && P.scalar_type() == torch::kFloat32 &&
              P.numel() > 0);
  const int64_t R = P.size(0), C = P.size(1);
  auto partials = torch::empty({(int64_t)filterbank_stats_partials(C)},
                               P.options().dtype(torch::kFloat64));
  auto mean = torch::empty({C}, P.options());
  auto stddev = torch::empty({C}, P.options());
  check(filterbank_channel_stats(P.data_ptr<float>(), R, C,
                                 partials.data_ptr<double>(),
                                 mean.data_ptr<float>(),
                                 stddev.data_ptr<float>(), cur_stream()),
        "filterbank_channel_stats");
  return {mean, stddev};
}

torch::Tensor t_filterbank_quantize(torch::Tensor P, torch::Tensor mean,
                                    torch::Tensor stddev) {
  CHECK_CUDA(P);
  CHECK_CONTIG(P);
  CHECK_CUDA(mean);
  CHECK_CONTIG(mean);
  CHECK_CUDA(stddev);
  CHECK_CONTIG(stddev);
  TORCH_CHECK(P.dim() == 2 && P.scalar_type() == torch::kFloat32 &&
              P.numel() > 0);
  const int64_t R = P.size(0), C = P.size(1);
  TORCH_CHECK(mean.scalar_type() == torch::kFloat32 && mean.numel() == C &&
              stddev.scalar_type() == torch::kFloat32 && stddev.numel() == C);
  auto out = torch::empty({R, C}, P.options().dtype(torch::kUInt8));
  check(filterbank_quantize(P.data_ptr<float>(), mean.data_ptr<float>(),
                            stddev.data_ptr<float>(), R, C,
                            out.data_ptr<uint8_t>(), cur_stream()),
        "filterbank_quantize");
  return out;
}

// ---------------- pulsar folding ----------------

// One fold_block() into caller-owned accumulators: acc float64 [S][nbin],
// hits [nbin] and weights [S] as 64-bit integer tensors (the bits are u64).
void t_fold_block(torch::Tensor wf, c10::optional<torch::Tensor> flags,
                  int64_t valid, int64_t nbin, uint64_t phi, uint64_t dphi,
                  torch::Tensor acc, torch::Tensor hits,
                  torch::Tensor weights) {
  CHECK_CUDA(wf);
  CHECK_CONTIG(wf);
  CHECK_CUDA(acc);
  CHECK_CONTIG(acc);
  CHECK_CUDA(hits);
  CHECK_CONTIG(hits);
  CHECK_CUDA(weights);
  CHECK_CONTIG(weights);
  TORCH_CHECK(wf.dim() == 2 && wf.scalar_type() == torch::kComplexFloat);
  const int64_t S = wf.size(0), L = wf.size(1);
  TORCH_CHECK(S >= 1 && valid >= 1 && valid <= L &&
                  nbin >= (int64_t)kFoldMinBins &&
                  nbin <= (int64_t)kFoldMaxBins,
              "fold_block: bad geometry");
  auto is_u64 = [](const torch::Tensor& t) {
    return t.scalar_type() == torch::kInt64 ||
           t.scalar_type() == torch::kUInt64;
  };
  TORCH_CHECK(acc.scalar_type() == torch::kFloat64 && acc.dim() == 2 &&
                  acc.size(0) == S && acc.size(1) == nbin,
              "fold_block: acc must be float64 [S][nbin]");
  TORCH_CHECK(is_u64(hits) && hits.dim() == 1 && hits.size(0) == nbin,
              "fold_block: hits must be 64-bit integer [nbin]");
  TORCH_CHECK(is_u64(weights) && weights.dim() == 1 && weights.size(0) == S,
              "fold_block: weights must be 64-bit integer [S]");
  const uint8_t* f = nullptr;
  if (flags.has_value()) {
    CHECK_CUDA(*flags);
    CHECK_CONTIG(*flags);
    TORCH_CHECK(flags->scalar_type() == torch::kUInt8 && flags->numel() == S);
    f = flags->data_ptr<uint8_t>();
  }
  auto words = torch::tensor({(int64_t)phi, (int64_t)dphi},
                             torch::TensorOptions().dtype(torch::kInt64))
                   .to(wf.device());
  auto table = torch::empty({(int64_t)fold_table_words(valid)},
                            wf.options().dtype(torch::kInt32));
  check(fold_block(cptr(wf), f, S, L, valid, nbin,
                   static_cast<const uint64_t*>(words.data_ptr()),
                   static_cast<uint32_t*>(table.data_ptr()),
                   acc.data_ptr<double>(),
                   static_cast<uint64_t*>(hits.data_ptr()),
                   static_cast<uint64_t*>(weights.data_ptr()), cur_stream()),
        "fold_block");
}

// ---------------- hand-written FFT (test/bench surface) ----------------

torch::Tensor t_native_fft(torch::Tensor x, int64_t sign) {
  CHECK_CUDA(x);
  CHECK_CONTIG(x);
  TORCH_CHECK(x.scalar_type() == torch::kComplexFloat);
  const size_t len = x.size(-1);
  const size_t batch = x.numel() / len;
  auto stream = cur_stream();
  NativeFft plan;
  plan.plan(len, batch, (int)sign, stream);
  auto out = torch::empty_like(x);
  if (plan.n_passes() == 1) {
    plan.exec(cptr(x), cptr(out), stream);
  } else {
    auto work = x.clone();  // passes 0..k-2 run in place on the input copy
    plan.exec(cptr(work), cptr(out), stream);
  }
  check(hipStreamSynchronize(stream), "native_fft sync");  // plan is local
  return out;
}

// Batched backward NativeFft of a [rows][len] tensor with the spectral-
// kurtosis sums accumulated in the final DIF pass's store, as the engine's
// waterfall transform runs it: (out, s2s4 float32 [rows][2]).
std::vector<torch::Tensor> t_native_fft_sk(torch::Tensor x) {
  CHECK_CUDA(x);
  CHECK_CONTIG(x);
  TORCH_CHECK(x.scalar_type() == torch::kComplexFloat && x.dim() == 2);
  const size_t rows = x.size(0), len = x.size(1);
  auto stream = cur_stream();
  NativeFft plan;
  plan.plan(len, rows, +1, stream);
  const int wpr = plan.dif_sk_wgs_per_row();
  TORCH_CHECK(wpr > 0, "native_fft_sk: the plan for length ", len,
              " has no fused spectral-kurtosis epilogue");
  auto partials = torch::empty({(int64_t)rows * wpr, 2},
                               x.options().dtype(torch::kFloat32));
  auto s2s4 = torch::empty({(int64_t)rows, 2},
                           x.options().dtype(torch::kFloat32));
  auto out = torch::empty_like(x);
  auto* pp = reinterpret_cast<float2*>(partials.data_ptr<float>());
  if (plan.n_passes() == 1) {
    plan.exec(cptr(x), cptr(out), stream, nullptr, pp);
  } else {
    auto work = x.clone();  // passes 0..k-2 run in place on the input copy
    plan.exec(cptr(work), cptr(out), stream, nullptr, pp);
  }
  check(sk_combine_partials(pp, rows, wpr,
                            reinterpret_cast<float2*>(s2s4.data_ptr<float>()),
                            stream),
        "sk_combine_partials");
  check(hipStreamSynchronize(stream), "native_fft_sk sync");  // plan is local
  return {out, s2s4};
}

// Batched backward NativeFft with the fused RFI + zap + dedispersion pre-op
// on its first pass, below engine level.  One plan runs once per entry of
// `dms` (the DM-sweep front end's usage); returns ([out per dm], [whether the
// column-polynomial phase path ran per dm]).
std::tuple<std::vector<torch::Tensor>, std::vector<bool>> t_preop_backward_fft(
    torch::Tensor spec, int64_t maxcol_log2, int64_t final_log2, double f_min,
    double f_c, double df, std::vector<double> dms,
    std::vector<std::vector<int64_t>> ranges, bool enable_rfi,
    double threshold, int64_t channel_count) {
  CHECK_CUDA(spec);
  CHECK_CONTIG(spec);
  TORCH_CHECK(spec.scalar_type() == torch::kComplexFloat);
  TORCH_CHECK(ranges.size() <= 16, "at most 16 zap ranges");
  const size_t len = spec.size(-1);
  const size_t n = spec.numel();
  const size_t batch = n / len;
  auto stream = cur_stream();
  NativeFft plan;
  plan.plan(len, batch, +1, stream, (int)maxcol_log2, (int)final_log2);
  TORCH_CHECK(plan.first_pass_fusable(), "plan has no column first pass");
  torch::Tensor mean;
  FftPreop pre;
  if (enable_rfi) {
    mean = t_mean_power(spec);
    pre.mean_power = mean.data_ptr<double>();
    pre.threshold = (float)threshold;
    pre.norm_coeff =
        (float)std::pow((double)n * (double)n / (double)channel_count, -0.5);
  }
  pre.n_zap = (int)ranges.size();
  for (size_t i = 0; i < ranges.size(); ++i) {
    pre.zap[i].lo = (unsigned long long)ranges[i][0];
    pre.zap[i].hi = (unsigned long long)ranges[i][1];
  }
  pre.f_min = f_min;
  pre.f_c = f_c;
  pre.df = df;
  std::vector<torch::Tensor> outs;
  std::vector<bool> poly;
  for (double dm : dms) {
    pre.dm = dm;
    poly.push_back(plan.preop_uses_poly(pre));
    auto work = spec.clone();  // the column passes run in place
    auto out = torch::empty_like(spec);
    plan.exec(cptr(work), cptr(out), stream, &pre);
    outs.push_back(out);
  }
  check(hipStreamSynchronize(stream), "preop_backward_fft sync");
  return {outs, poly};
}

torch::Tensor t_dedisp_poly_factors(int64_t nc, int64_t n, int64_t stride,
                                    double f_min, double f_c, double df,
                                    double dm, torch::Device dev) {
  auto out = torch::empty({nc}, torch::TensorOptions()
                                    .dtype(torch::kComplexFloat)
                                    .device(dev));
  check(dedisp_poly_factors(cptr(out), (size_t)nc, (uint32_t)n,
                            (size_t)stride, f_min, f_c, df, dm, cur_stream()),
        "dedisp_poly_factors");
  return out;
}

torch::Tensor t_native_rfft(torch::Tensor x) {
  // real forward via packed-complex trick + r2c post; returns n/2 bins
  CHECK_CUDA(x);
  CHECK_CONTIG(x);
  TORCH_CHECK(x.scalar_type() == torch::kFloat32);
  const size_t n = x.numel();
  const size_t m = n / 2;
  auto stream = cur_stream();
  NativeFft plan;
  plan.plan(m, 1, -1, stream);
  auto z = torch::empty({(int64_t)m},
                        x.options().dtype(torch::kComplexFloat));
  auto packed = x.view({(int64_t)m, 2});  // reinterpret as complex pairs
  auto work = torch::empty_like(z);
  work.copy_(torch::view_as_complex(packed));
  if (plan.r2c_final_partials()) {
    // the final pass combines the (k, m-k) pairs at its store
    const NativeFft::R2cFinal rf;
    plan.exec(cptr(work), cptr(z), stream, nullptr, nullptr, nullptr, 2,
              nullptr, &rf);
  } else {
    plan.exec(cptr(work), cptr(z), stream);
    check(r2c_post_process(cptr(z), cptr(z), m, nullptr, nullptr, stream),
          "r2c post");
  }
  check(hipStreamSynchronize(stream), "native_rfft sync");
  return z;
}

// native_rfft of the samples that `raw` holds at `nbits`, decoded in the
// first column pass's loads (the engine's default front half): the same plan
// and the same ending as native_rfft for numel * 8 / |nbits| samples, and no
// unpacked sample buffer beyond the in-place work area.
torch::Tensor t_native_rfft_raw(torch::Tensor raw, int64_t nbits) {
  CHECK_CUDA(raw);
  CHECK_CONTIG(raw);
  TORCH_CHECK(raw.scalar_type() == torch::kUInt8);
  const int64_t ab = std::abs(nbits);
  TORCH_CHECK(ab == 1 || ab == 2 || ab == 4 || ab == 8 || ab == 16,
              "native_rfft_raw: nbits must be 1, 2, 4, 8, -8, 16 or -16");
  TORCH_CHECK(nbits > 0 || ab >= 8, "native_rfft_raw: no signed sub-byte");
  const size_t n = (size_t)raw.numel() * 8 / (size_t)ab;
  const size_t m = n / 2;
  TORCH_CHECK(m >= 2 && m * 2 * (size_t)ab == (size_t)raw.numel() * 8,
              "native_rfft_raw: raw must hold an even number of samples");
  auto stream = cur_stream();
  NativeFft plan;
  plan.plan(m, 1, -1, stream);
  TORCH_CHECK(plan.first_pass_fusable(), "native_rfft_raw: the plan for ", m,
              " complex elements has no column first pass");
  auto z = torch::empty({(int64_t)m},
                        raw.options().dtype(torch::kComplexFloat));
  auto work = torch::empty_like(z);  // written by the decoding first pass
  const uint8_t* rp = raw.data_ptr<uint8_t>();
  if (plan.r2c_final_partials()) {
    const NativeFft::R2cFinal rf;
    plan.exec(cptr(work), cptr(z), stream, nullptr, nullptr, rp, (int)nbits,
              nullptr, &rf);
  } else {
    plan.exec(cptr(work), cptr(z), stream, nullptr, nullptr, rp, (int)nbits);
    check(r2c_post_process(cptr(z), cptr(z), m, nullptr, nullptr, stream),
          "r2c post");
  }
  check(hipStreamSynchronize(stream), "native_rfft_raw sync");
  return z;
}

int64_t t_native_rfft_final_partials(int64_t n) {
  // what native_rfft's plan for n real samples reports: > 0 = its final pass
  // does the r2c pair-combine (and would write that many mean partials)
  auto stream = cur_stream();
  NativeFft plan;
  plan.plan((size_t)n / 2, 1, -1, stream);
  check(hipStreamSynchronize(stream), "native_rfft plan sync");
  return plan.r2c_final_partials();
}

// ---------------- FFT microbenchmarks (plan once, event-timed) ----------------

double time_iters(hipStream_t stream, int iters, const std::function<void()>& f) {
  hipEvent_t e0, e1;
  check(hipEventCreate(&e0), "ev");
  check(hipEventCreate(&e1), "ev");
  f();  // warmup
  check(hipStreamSynchronize(stream), "warm sync");
  check(hipEventRecord(e0, stream), "rec");
  for (int i = 0; i < iters; ++i) f();
  check(hipEventRecord(e1, stream), "rec");
  check(hipEventSynchronize(e1), "sync");
  float ms = 0;
  check(hipEventElapsedTime(&ms, e0, e1), "elapsed");
  hipEventDestroy(e0);
  hipEventDestroy(e1);
  return ms / iters;
}

double t_bench_fft(int64_t len, int64_t batch, int64_t sign, int64_t iters,
                   std::string backend) {
  auto stream = cur_stream();
  auto x = torch::randn({batch, len, 2},
                        torch::TensorOptions().dtype(torch::kFloat32)
                            .device(torch::kCUDA));
  auto y = torch::empty_like(x);
  float2* xp = reinterpret_cast<float2*>(x.data_ptr());
  float2* yp = reinterpret_cast<float2*>(y.data_ptr());
  double ms = 0;
  if (backend == "native") {
    NativeFft plan;
    plan.plan(len, batch, (int)sign, stream);
    ms = time_iters(stream, (int)iters, [&] { plan.exec(xp, yp, stream); });
  } else {
    hipfftHandle h;
    check_fft(hipfftCreate(&h), "create");
    long long n1[1] = {(long long)len};
    size_t ws = 0;
    check_fft(hipfftMakePlanMany64(h, 1, n1, nullptr, 1, len, nullptr, 1, len,
                                   HIPFFT_C2C, batch, &ws),
              "plan");
    check_fft(hipfftSetStream(h, stream), "stream");
    ms = time_iters(stream, (int)iters, [&] {
      hipfftExecC2C(h, reinterpret_cast<hipfftComplex*>(xp),
                    reinterpret_cast<hipfftComplex*>(yp),
                    sign < 0 ? HIPFFT_FORWARD : HIPFFT_BACKWARD);
    });
    hipfftDestroy(h);
  }
  return ms;
}

double t_bench_rfft(int64_t n, int64_t iters, std::string backend) {
  auto stream = cur_stream();
  auto x = torch::randn({n}, torch::TensorOptions()
                                 .dtype(torch::kFloat32)
                                 .device(torch::kCUDA));
  auto y = torch::empty({n / 2 + 1, 2}, x.options());
  float* xp = x.data_ptr<float>();
  float2* yp = reinterpret_cast<float2*>(y.data_ptr());
  double ms = 0;
  if (backend == "native") {
    const size_t m = n / 2;
    NativeFft plan;
    plan.plan(m, 1, -1, stream);
    const bool fused = plan.r2c_final_partials() != 0;
    const NativeFft::R2cFinal rf;
    ms = time_iters(stream, (int)iters, [&] {
      if (fused) {
        plan.exec(reinterpret_cast<float2*>(xp), yp, stream, nullptr, nullptr,
                  nullptr, 2, nullptr, &rf);
      } else {
        plan.exec(reinterpret_cast<float2*>(xp), yp, stream);
        check(r2c_post_process(yp, yp, m, nullptr, nullptr, stream), "post");
      }
    });
  } else {
    hipfftHandle h;
    check_fft(hipfftCreate(&h), "create");
    long long n1[1] = {(long long)n};
    size_t ws = 0;
    check_fft(hipfftMakePlanMany64(h, 1, n1, nullptr, 1, 0, nullptr, 1, 0,
                                   HIPFFT_R2C, 1, &ws),
              "plan");
    check_fft(hipfftSetStream(h, stream), "stream");
    ms = time_iters(stream, (int)iters, [&] {
      hipfftExecR2C(h, xp, reinterpret_cast<hipfftComplex*>(yp));
    });
    hipfftDestroy(h);
  }
  return ms;
}

// ---------------- engine binding ----------------

class PyEngine {
 public:
  PyEngine(int64_t n, int64_t nbits, int64_t channels, double freq_low,
           double bandwidth, double sample_rate, double dm,
           double rfi_threshold, double sk_threshold, double snr_threshold,
           int64_t max_boxcar, int64_t nsamps_reserved,
           std::vector<std::vector<int64_t>> zap_ranges, bool use_phase_table,
           bool enable_rfi_s1, bool enable_sk, int64_t n_slots,
           int64_t fft_backend, int64_t window_kind, bool use_hip_graph,
           int64_t max_dm_trials, int64_t fil_tscrunch, int64_t fil_fscrunch,
           int64_t fil_nbits, int64_t fold_nbin, double fold_f0,
           double fold_f1, double fold_phase0) {
    EngineConfig c;
    c.baseband_input_count = n;
    c.baseband_input_bits = (int)nbits;
    c.spectrum_channel_count = channels;
    c.freq_low = freq_low;
    c.bandwidth = bandwidth;
    c.sample_rate = sample_rate;
    c.dm = dm;
    c.rfi_threshold = (float)rfi_threshold;
    c.sk_threshold = (float)sk_threshold;
    c.snr_threshold = (float)snr_threshold;
    c.max_boxcar_length = max_boxcar;
    c.nsamps_reserved = nsamps_reserved;
    TORCH_CHECK(zap_ranges.size() <= 16);
    c.n_zap_ranges = (int)zap_ranges.size();
    for (size_t i = 0; i < zap_ranges.size(); ++i) {
      c.zap_ranges[i].lo = (unsigned long long)zap_ranges[i][0];
      c.zap_ranges[i].hi = (unsigned long long)zap_ranges[i][1];
    }
    c.use_phase_table = use_phase_table;
    c.enable_rfi_s1 = enable_rfi_s1;
    c.enable_sk = enable_sk;
    c.fft_backend = (int)fft_backend;
    c.window_kind = (int)window_kind;
    c.use_hip_graph = use_hip_graph;
    c.max_dm_trials = (int)max_dm_trials;
    TORCH_CHECK(fil_tscrunch >= 0 && fil_fscrunch >= 0,
                "fil_tscrunch and fil_fscrunch must not be negative");
    c.fil_tscrunch = (size_t)fil_tscrunch;
    c.fil_fscrunch = (size_t)fil_fscrunch;
    c.fil_nbits = (int)fil_nbits;
    TORCH_CHECK(fold_nbin >= 0, "fold_nbin must not be negative");
    c.fold_nbin = (size_t)fold_nbin;
    c.fold_f0 = fold_f0;
    c.fold_f1 = fold_f1;
    c.fold_phase0 = fold_phase0;
    eng_ = std::make_unique<PipelineEngine>(c, (int)n_slots);
  }

  // device-tensor submissions: the tensor was produced on torch's current
  // stream while the engine enqueues on its own slot stream — record a
  // producer event and have the slot stream wait on it (no host sync)
  hipEvent_t producer_event() {
    if (!prod_ev_)
      check(hipEventCreateWithFlags(&prod_ev_, hipEventDisableTiming),
            "producer event create");
    check(hipEventRecord(prod_ev_, cur_stream()), "producer event record");
    return prod_ev_;
  }

  int64_t submit(torch::Tensor raw, double dm_override) {
    TORCH_CHECK(raw.is_contiguous());
    TORCH_CHECK((size_t)raw.numel() * raw.element_size() == eng_->raw_bytes(),
                "raw block has wrong byte size");
    if (raw.is_cuda())
      return eng_->submit_device(raw.data_ptr(), eng_->raw_bytes(),
                                 dm_override, producer_event());
    return eng_->submit(raw.data_ptr(), eng_->raw_bytes(), dm_override);
  }

  int64_t submit_samples(torch::Tensor samples, double dm_override) {
    TORCH_CHECK(samples.is_cuda() && samples.is_contiguous());
    TORCH_CHECK(samples.scalar_type() == torch::kFloat32);
    return eng_->submit_samples_device(samples.data_ptr<float>(),
                                       samples.numel(), dm_override,
                                       producer_event());
  }

  int64_t submit_trials(torch::Tensor raw, std::vector<double> dms) {
    TORCH_CHECK(raw.is_contiguous());
    TORCH_CHECK((size_t)raw.numel() * raw.element_size() == eng_->raw_bytes(),
                "raw block has wrong byte size");
    if (raw.is_cuda())
      return eng_->submit_trials_device(raw.data_ptr(), eng_->raw_bytes(),
                                        dms.data(), (int)dms.size(),
                                        producer_event());
    return eng_->submit_trials(raw.data_ptr(), eng_->raw_bytes(), dms.data(),
                               (int)dms.size());
  }

  int64_t submit_trials_samples(torch::Tensor samples,
                                std::vector<double> dms) {
    TORCH_CHECK(samples.is_cuda() && samples.is_contiguous());
    TORCH_CHECK(samples.scalar_type() == torch::kFloat32);
    return eng_->submit_trials_samples_device(
        samples.data_ptr<float>(), samples.numel(), dms.data(),
        (int)dms.size(), producer_event());
  }

  static py::dict result_dict(const BlockResult& r) {
    py::dict d;
    d["zero_count"] = r.zero_count;
    py::list counts;
    for (auto& c : r.counts) counts.append(py::make_tuple(c.first, c.second));
    d["counts"] = counts;
    py::list thr;
    for (float t : r.thresholds) thr.append(t);
    d["thresholds"] = thr;
    return d;
  }

  py::dict wait(int64_t slot) { return result_dict(eng_->wait((int)slot)); }

  // one dict per trial: wait()'s keys plus "dm" and "peaks", a list of
  // {boxcar_length, value, index, snr} (raw series first)
  py::list wait_trials(int64_t slot) {
    py::list out;
    for (const auto& t : eng_->wait_trials((int)slot)) {
      py::dict d = result_dict(t.result);
      d["dm"] = t.dm;
      py::list peaks;
      for (const auto& p : t.peaks) {
        py::dict pd;
        pd["boxcar_length"] = p.boxcar_length;
        pd["value"] = p.value;
        pd["index"] = p.index;
        pd["snr"] = p.snr;
        peaks.append(pd);
      }
      d["peaks"] = peaks;
      out.append(d);
    }
    return out;
  }

  // blocks until the re-run has finished
  void select_trial(int64_t slot, int64_t k) {
    eng_->select_trial((int)slot, (int)k);
    check(hipStreamSynchronize(eng_->stream((int)slot)), "select_trial sync");
  }

  torch::Tensor dm_time_plane(int64_t slot) {
    return torch::from_blob(eng_->dm_time_plane_ptr((int)slot),
                            {(int64_t)eng_->n_trials((int)slot),
                             (int64_t)eng_->ts_count()},
                            torch::TensorOptions()
                                .dtype(torch::kFloat32)
                                .device(torch::kCUDA));
  }

  torch::Tensor cumsum(int64_t slot) {
    return torch::from_blob(eng_->cumsum_ptr((int)slot),
                            {(int64_t)eng_->ts_count()},
                            torch::TensorOptions()
                                .dtype(torch::kFloat32)
                                .device(torch::kCUDA));
  }

  void synchronize() { eng_->synchronize(); }

  // zap = false (test surface): a COPY of the waterfall as the chain left
  // it, without triggering the deferred spectral-kurtosis row zap
  torch::Tensor waterfall(int64_t slot, bool zap) {
    const auto S = (int64_t)eng_->n_channels(), L = (int64_t)eng_->waterfall_len();
    const auto opt = torch::TensorOptions()
                         .dtype(torch::kComplexFloat)
                         .device(torch::kCUDA);
    if (!zap) {
      sync_slot(slot);
      return torch::from_blob(
                 const_cast<float2*>(eng_->waterfall_unzapped_ptr((int)slot)),
                 {S, L}, opt)
          .clone();
    }
    return torch::from_blob(eng_->waterfall_ptr((int)slot), {S, L}, opt);
  }

  void sync_slot(int64_t slot) {
    check(hipStreamSynchronize(eng_->stream((int)slot)), "slot sync");
  }

  // [S][2] float32 copy of the slot's <sum|x|^2, sum|x|^4> (test surface)
  torch::Tensor sk_stats(int64_t slot) {
    const float2* p = eng_->sk_stats_ptr((int)slot);
    TORCH_CHECK(p, "sk_stats: the engine was built with enable_sk = false");
    sync_slot(slot);
    return torch::from_blob(const_cast<float2*>(p),
                            {(int64_t)eng_->n_channels(), 2},
                            torch::TensorOptions()
                                .dtype(torch::kFloat32)
                                .device(torch::kCUDA))
        .clone();
  }

  // [S] uint8 copy of the slot's spectral-kurtosis flags (test surface)
  torch::Tensor sk_flags(int64_t slot) {
    const uint8_t* p = eng_->sk_flags_ptr((int)slot);
    TORCH_CHECK(p, "sk_flags: the engine was built with enable_sk = false");
    sync_slot(slot);
    return torch::from_blob(const_cast<uint8_t*>(p),
                            {(int64_t)eng_->n_channels()},
                            torch::TensorOptions()
                                .dtype(torch::kUInt8)
                                .device(torch::kCUDA))
        .clone();
  }

  torch::Tensor time_series(int64_t slot) {
    return torch::from_blob(eng_->time_series_ptr((int)slot),
                            {(int64_t)eng_->ts_count()},
                            torch::TensorOptions()
                                .dtype(torch::kFloat32)
                                .device(torch::kCUDA));
  }

  torch::Tensor boxcar_series(int64_t slot, int64_t L) {
    float* p = eng_->compute_boxcar((int)slot, L);
    auto t = torch::from_blob(p, {(int64_t)(eng_->ts_count() - L)},
                              torch::TensorOptions()
                                  .dtype(torch::kFloat32)
                                  .device(torch::kCUDA));
    return t.clone();
  }

  // [R][C] uint8 or float32: a copy of the slot's pinned mirror, complete
  // after wait(slot)
  torch::Tensor filterbank(int64_t slot) {
    const auto R = (int64_t)eng_->filterbank_rows(),
               C = (int64_t)eng_->filterbank_channels();
    const void* p = eng_->filterbank_host((int)slot);
    const auto dt = eng_->filterbank_nbits() == 8 ? torch::kUInt8
                                                  : torch::kFloat32;
    return torch::from_blob(const_cast<void*>(p), {R, C},
                            torch::TensorOptions().dtype(dt))
        .clone();
  }

  torch::Tensor filterbank_power(int64_t slot) {
    return torch::from_blob(eng_->filterbank_power_ptr((int)slot),
                            {(int64_t)eng_->filterbank_rows(),
                             (int64_t)eng_->filterbank_channels()},
                            torch::TensorOptions()
                                .dtype(torch::kFloat32)
                                .device(torch::kCUDA));
  }

  // (mean, std) per channel, CPU float32 (8-bit output only)
  std::vector<torch::Tensor> filterbank_stats(int64_t slot) {
    const auto C = (int64_t)eng_->filterbank_channels();
    auto opt = torch::TensorOptions().dtype(torch::kFloat32);
    auto mean = torch::from_blob(
        const_cast<float*>(eng_->filterbank_mean_host((int)slot)), {C}, opt);
    auto stddev = torch::from_blob(
        const_cast<float*>(eng_->filterbank_std_host((int)slot)), {C}, opt);
    return {mean.clone(), stddev.clone()};
  }

  void set_fold_next_sample(uint64_t n0) { eng_->set_fold_next_sample(n0); }
  uint64_t fold_next_sample() const { return eng_->fold_next_sample(); }

  // (n0, Phi_b, dPhi_b) of the slot's last submission, Python integers
  py::tuple fold_words(int64_t slot) {
    const auto w = eng_->fold_words((int)slot);
    return py::make_tuple(py::int_(w.n0), py::int_(w.phi), py::int_(w.dphi));
  }

  void fold_reset() { eng_->fold_reset(); }

  // Synchronises the engine.  (acc float64 [S][nbin], hits uint64 [nbin],
  // weights uint64 [S]) as NumPy arrays, the slots summed in slot order.
  py::tuple fold_read() {
    const auto S = (py::ssize_t)eng_->n_channels(),
               nb = (py::ssize_t)eng_->fold_nbin();
    py::array_t<double> acc({S, nb});
    py::array_t<uint64_t> hits(nb), weights(S);
    eng_->fold_read(acc.mutable_data(), hits.mutable_data(),
                    weights.mutable_data());
    return py::make_tuple(acc, hits, weights);
  }

  int64_t filterbank_rows() const { return eng_->filterbank_rows(); }
  int64_t filterbank_channels() const { return eng_->filterbank_channels(); }

  PipelineEngine& engine() { return *eng_; }

  int64_t n() const { return eng_->n(); }
  int64_t nc() const { return eng_->nc(); }
  int64_t n_channels() const { return eng_->n_channels(); }
  int64_t waterfall_len() const { return eng_->waterfall_len(); }
  int64_t ts_count() const { return eng_->ts_count(); }
  int64_t raw_bytes() const { return eng_->raw_bytes(); }
  int64_t n_slots() const { return eng_->n_slots(); }

 private:
  std::unique_ptr<PipelineEngine> eng_;
  hipEvent_t prod_ev_ = nullptr;

 public:
  ~PyEngine() {
    if (prod_ev_) (void)hipEventDestroy(prod_ev_);
  }
};

// ---------------- polarization combiner binding ----------------

class PyPolCombiner {
 public:
  PyPolCombiner(int64_t n, int64_t channels, int64_t nsamps_reserved,
                int64_t tscrunch, int64_t fscrunch, bool reverse,
                int64_t pol_state, int64_t nbits, int64_t n_slots) {
    TORCH_CHECK(n >= 0 && channels >= 0 && nsamps_reserved >= 0 &&
                    tscrunch >= 0 && fscrunch >= 0,
                "PolCombiner: sizes must not be negative");
    PolCombinerConfig c;
    c.baseband_input_count = (size_t)n;
    c.spectrum_channel_count = (size_t)channels;
    c.nsamps_reserved = (size_t)nsamps_reserved;
    c.tscrunch = (size_t)tscrunch;
    c.fscrunch = (size_t)fscrunch;
    c.reverse = reverse;
    c.pol_state = (int)pol_state;
    c.nbits = (int)nbits;
    comb_ = std::make_unique<PolCombiner>(c, (int)n_slots);
  }

  int64_t submit(PyEngine& a, int64_t slot_a, PyEngine& b, int64_t slot_b) {
    return comb_->submit(a.engine(), (int)slot_a, b.engine(), (int)slot_b);
  }

  void wait(int64_t k) { comb_->wait((int)k); }

  std::vector<int64_t> shape() const {
    return {(int64_t)comb_->rows(), (int64_t)comb_->nifs(),
            (int64_t)comb_->channels()};
  }

  // [R][P][C] uint8 or float32: a copy of the slot's pinned mirror, complete
  // after wait(k)
  torch::Tensor plane(int64_t k) {
    const auto dt = comb_->nbits() == 8 ? torch::kUInt8 : torch::kFloat32;
    return torch::from_blob(const_cast<void*>(comb_->host((int)k)), shape(),
                            torch::TensorOptions().dtype(dt))
        .clone();
  }

  torch::Tensor power(int64_t k) {
    return torch::from_blob(comb_->power_ptr((int)k), shape(),
                            torch::TensorOptions()
                                .dtype(torch::kFloat32)
                                .device(torch::kCUDA));
  }

  // (mean, std) per (product, channel), CPU float32 [P * C] (8-bit only)
  std::vector<torch::Tensor> stats(int64_t k) {
    const auto pc = (int64_t)comb_->nifs() * (int64_t)comb_->channels();
    auto opt = torch::TensorOptions().dtype(torch::kFloat32);
    auto mean = torch::from_blob(
        const_cast<float*>(comb_->mean_host((int)k)), {pc}, opt);
    auto stddev = torch::from_blob(
        const_cast<float*>(comb_->std_host((int)k)), {pc}, opt);
    return {mean.clone(), stddev.clone()};
  }

  int64_t rows() const { return comb_->rows(); }
  int64_t channels() const { return comb_->channels(); }
  int64_t nifs() const { return comb_->nifs(); }

 private:
  std::unique_ptr<PolCombiner> comb_;
};

// ---------------- incoherent DM-offset search bindings ----------------

// Y float32 [T][R] of a linear window [D_max + R][C] and a table [T][C] int32
torch::Tensor t_incoh_dedisperse(torch::Tensor window, torch::Tensor delays,
                                 int64_t R) {
  CHECK_CUDA(window);
  CHECK_CUDA(delays);
  CHECK_CONTIG(window);
  CHECK_CONTIG(delays);
  TORCH_CHECK(window.scalar_type() == torch::kFloat32 && window.dim() == 2,
              "incoh_dedisperse: window must be float32 [D_max + R][C]");
  TORCH_CHECK(delays.scalar_type() == torch::kInt32 && delays.dim() == 2,
              "incoh_dedisperse: delays must be int32 [T][C]");
  const int64_t rows = window.size(0), C = window.size(1), T = delays.size(0);
  TORCH_CHECK(T >= 1 && T <= (int64_t)kIncohMaxTrials,
              "incoh_dedisperse: needs 1 .. ", kIncohMaxTrials, " trials");
  TORCH_CHECK(C >= 1 && delays.size(1) == C,
              "incoh_dedisperse: window and delays differ in channels");
  TORCH_CHECK(R >= (int64_t)kIncohMinRows && R <= rows,
              "incoh_dedisperse: R must be ", kIncohMinRows,
              " .. the window's ", rows, " rows");
  const int64_t d_max = rows - R;
  TORCH_CHECK(d_max <= (int64_t)kIncohMaxDelay &&
                  (size_t)rows * (size_t)C * sizeof(float) <=
                      kIncohMaxWindowBytes,
              "incoh_dedisperse: the window exceeds the limits (D_max <= ",
              kIncohMaxDelay, ", at most ", kIncohMaxWindowBytes, " bytes)");
  // the kernel trusts the table: look at it here (one small reduction)
  const int64_t lo = delays.min().item<int64_t>(),
                hi = delays.max().item<int64_t>();
  TORCH_CHECK(lo >= 0 && hi <= d_max, "incoh_dedisperse: delays must lie in ",
              "0 .. ", d_max, ", found ", lo, " .. ", hi);
  auto Y = torch::empty({T, R}, window.options());
  torch::Tensor partials;
  float* pp = nullptr;
  if (const size_t np = incoh_partials(T, R, C)) {
    partials = torch::empty({(int64_t)np}, window.options());
    pp = partials.data_ptr<float>();
  }
  check(incoh_dedisperse(window.data_ptr<float>(), rows, 0,
                         delays.data_ptr<int>(), T, R, C, pp,
                         Y.data_ptr<float>(), cur_stream()),
        "incoh_dedisperse");
  return Y;
}

// (peak float64 [T][NL], index int64 [T][NL] (-1: no window), rms float64
// [T][NL], count int64 [T][NL], mu float64 [T]) for lengths 1, 2, 4 ...
// max_boxcar
std::vector<torch::Tensor> t_incoh_detect(torch::Tensor Y, double snr,
                                          int64_t max_boxcar) {
  CHECK_CUDA(Y);
  CHECK_CONTIG(Y);
  TORCH_CHECK(Y.scalar_type() == torch::kFloat32 && Y.dim() == 2,
              "incoh_detect: Y must be float32 [T][R]");
  const int64_t T = Y.size(0), R = Y.size(1);
  TORCH_CHECK(T >= 1 && T <= (int64_t)kIncohMaxTrials,
              "incoh_detect: needs 1 .. ", kIncohMaxTrials, " trials");
  TORCH_CHECK(R >= (int64_t)kIncohMinRows && R <= (int64_t)kIncohMaxRows,
              "incoh_detect: R must be ", kIncohMinRows, " .. ",
              kIncohMaxRows);
  TORCH_CHECK(max_boxcar >= 1, "incoh_detect: max_boxcar must be >= 1");
  const int nl = incoh_lengths((size_t)max_boxcar);
  auto f64 = Y.options().dtype(torch::kFloat64);
  auto i32 = Y.options().dtype(torch::kInt32);
  auto peak = torch::empty({T, nl}, f64), rms = torch::empty({T, nl}, f64);
  auto mu = torch::empty({T}, f64);
  auto index = torch::empty({T, nl}, i32), count = torch::empty({T, nl}, i32);
  check(incoh_detect(Y.data_ptr<float>(), T, R, nl, snr,
                     peak.data_ptr<double>(),
                     reinterpret_cast<unsigned*>(index.data_ptr<int>()),
                     rms.data_ptr<double>(),
                     reinterpret_cast<unsigned*>(count.data_ptr<int>()),
                     mu.data_ptr<double>(), cur_stream()),
        "incoh_detect");
  // UINT_MAX reads as -1 through int32
  return {peak, index.to(torch::kInt64), rms, count.to(torch::kInt64), mu};
}

// One step of the normalisation state on a block plane [R][C]: M, V (float64
// [C]) and G (float32 [C]) are updated in place; returns the live count.
int64_t t_incoh_norm_update(torch::Tensor plane, double alpha,
                            torch::Tensor M, torch::Tensor V,
                            torch::Tensor G) {
  for (const torch::Tensor& t : {plane, M, V, G}) {
    CHECK_CUDA(t);
    CHECK_CONTIG(t);
  }
  TORCH_CHECK(plane.scalar_type() == torch::kFloat32 && plane.dim() == 2 &&
                  plane.size(0) >= 1 && plane.size(1) >= 1,
              "incoh_norm_update: plane must be float32 [R][C], R, C >= 1");
  const int64_t R = plane.size(0), C = plane.size(1);
  TORCH_CHECK(M.scalar_type() == torch::kFloat64 &&
                  V.scalar_type() == torch::kFloat64 && M.dim() == 1 &&
                  V.dim() == 1 && M.size(0) == C && V.size(0) == C,
              "incoh_norm_update: M and V must be float64 [C]");
  TORCH_CHECK(G.scalar_type() == torch::kFloat32 && G.dim() == 1 &&
                  G.size(0) == C,
              "incoh_norm_update: G must be float32 [C]");
  TORCH_CHECK(plane.device() == M.device() && M.device() == V.device() &&
                  V.device() == G.device(),
              "incoh_norm_update: tensors on different devices");
  TORCH_CHECK(alpha > 0.0 && alpha <= 1.0,
              "incoh_norm_update: alpha must be in (0, 1]");
  auto partials = torch::empty({(int64_t)incoh_norm_partials(C)},
                               plane.options().dtype(torch::kFloat64));
  auto live = torch::empty({1}, plane.options().dtype(torch::kInt32));
  check(incoh_norm_update(plane.data_ptr<float>(), R, C, alpha,
                          partials.data_ptr<double>(), M.data_ptr<double>(),
                          V.data_ptr<double>(), G.data_ptr<float>(),
                          reinterpret_cast<unsigned*>(live.data_ptr<int>()),
                          cur_stream()),
        "incoh_norm_update");
  return live.item<int64_t>();
}

// ring[(write_row + r) mod rows] = (plane[r] - (float)M) * G, in place
void t_incoh_norm_apply(torch::Tensor plane, torch::Tensor M, torch::Tensor G,
                        torch::Tensor ring, int64_t write_row) {
  for (const torch::Tensor& t : {plane, M, G, ring}) {
    CHECK_CUDA(t);
    CHECK_CONTIG(t);
  }
  TORCH_CHECK(plane.scalar_type() == torch::kFloat32 && plane.dim() == 2 &&
                  plane.size(0) >= 1 && plane.size(1) >= 1,
              "incoh_norm_apply: plane must be float32 [R][C], R, C >= 1");
  const int64_t R = plane.size(0), C = plane.size(1);
  TORCH_CHECK(M.scalar_type() == torch::kFloat64 && M.dim() == 1 &&
                  M.size(0) == C,
              "incoh_norm_apply: M must be float64 [C]");
  TORCH_CHECK(G.scalar_type() == torch::kFloat32 && G.dim() == 1 &&
                  G.size(0) == C,
              "incoh_norm_apply: G must be float32 [C]");
  TORCH_CHECK(ring.scalar_type() == torch::kFloat32 && ring.dim() == 2 &&
                  ring.size(1) == C && ring.size(0) >= R,
              "incoh_norm_apply: ring must be float32 [rows >= R][C]");
  TORCH_CHECK(write_row >= 0 && write_row < ring.size(0),
              "incoh_norm_apply: write_row must be in 0 .. rows - 1");
  TORCH_CHECK(plane.device() == M.device() && M.device() == G.device() &&
                  G.device() == ring.device(),
              "incoh_norm_apply: tensors on different devices");
  check(incoh_norm_apply(plane.data_ptr<float>(), R, C, M.data_ptr<double>(),
                         G.data_ptr<float>(), ring.data_ptr<float>(),
                         ring.size(0), write_row, cur_stream()),
        "incoh_norm_apply");
}

class PyIncoherentSearch {
 public:
  PyIncoherentSearch(int64_t rows, int64_t channels, double fch1, double foff,
                     double tsamp, std::vector<double> offsets,
                     double snr_threshold, int64_t max_boxcar,
                     int64_t n_slots, bool normalize,
                     int64_t normalize_blocks) {
    TORCH_CHECK(rows >= 0 && channels >= 0 && max_boxcar >= 0,
                "IncoherentSearch: sizes must not be negative");
    TORCH_CHECK(normalize_blocks >= 0,
                "IncoherentSearch: normalize_blocks must be 1 .. ",
                kIncohNormMaxBlocks);
    IncoherentSearchConfig c;
    c.rows = (size_t)rows;
    c.channels = (size_t)channels;
    c.fch1 = fch1;
    c.foff = foff;
    c.tsamp = tsamp;
    c.offsets = std::move(offsets);
    c.snr_threshold = snr_threshold;
    c.max_boxcar = (size_t)max_boxcar;
    c.normalize = normalize;
    c.normalize_blocks = (size_t)normalize_blocks;
    s_ = std::make_unique<IncoherentSearch>(c, (int)n_slots);
    check(hipEventCreateWithFlags(&ev_, hipEventDisableTiming),
          "incoherent producer event");
  }
  ~PyIncoherentSearch() {
    s_.reset();
    if (ev_) (void)hipEventDestroy(ev_);
  }

  int64_t submit(PyEngine& eng, int64_t slot) {
    return s_->submit(eng.engine(), (int)slot);
  }

  // plane: float32 [R][C] on the GPU, produced on the current torch stream;
  // it must stay alive and unchanged until wait(k)
  int64_t submit_plane(torch::Tensor plane) {
    CHECK_CUDA(plane);
    CHECK_CONTIG(plane);
    TORCH_CHECK(plane.scalar_type() == torch::kFloat32 && plane.dim() == 2 &&
                    plane.size(0) == (int64_t)s_->rows() &&
                    plane.size(1) == (int64_t)s_->channels(),
                "IncoherentSearch: plane must be float32 [", s_->rows(), "][",
                s_->channels(), "]");
    check(hipEventRecord(ev_, cur_stream()), "incoherent producer record");
    return s_->submit_plane(plane.data_ptr<float>(), ev_);
  }

  // {valid, first_row, block, live_channels, trials: [{offset, mean, lengths:
  // [{boxcar_length, peak, index, rms, count, snr}]}]}
  py::dict wait(int64_t k) {
    const IncoherentResult r = s_->wait((int)k);
    py::dict d;
    d["valid"] = r.valid;
    d["first_row"] = r.first_row;
    d["block"] = r.block;
    d["live_channels"] = r.live_channels;
    py::list trials;
    for (const IncoherentTrial& t : r.trials) {
      py::dict td;
      td["offset"] = t.offset;
      td["mean"] = t.mean;
      py::list ls;
      for (const IncoherentDetection& l : t.lengths) {
        py::dict ld;
        ld["boxcar_length"] = l.boxcar_length;
        ld["peak"] = l.peak;
        ld["index"] = l.index == 0xFFFFFFFFu ? (int64_t)-1 : (int64_t)l.index;
        ld["rms"] = l.rms;
        ld["count"] = l.count;
        ld["snr"] = l.snr;
        ls.append(ld);
      }
      td["lengths"] = ls;
      trials.append(td);
    }
    d["trials"] = trials;
    return d;
  }

  // [T][R] float32: a copy of the slot's pinned mirror, complete after wait(k)
  torch::Tensor plane(int64_t k) {
    return torch::from_blob(const_cast<float*>(s_->plane_host((int)k)),
                            {(int64_t)s_->trials(), (int64_t)s_->rows()},
                            torch::TensorOptions().dtype(torch::kFloat32))
        .clone();
  }

  // [T][C] int32 on the CPU
  torch::Tensor delays() {
    const auto& d = s_->delays();
    return torch::from_blob(const_cast<int32_t*>(d.data()),
                            {(int64_t)s_->trials(), (int64_t)s_->channels()},
                            torch::TensorOptions().dtype(torch::kInt32))
        .clone();
  }

  // the normalisation's running state, [C], copied once everything submitted
  // so far has run
  torch::Tensor norm_mean() { return norm_state(s_->norm_mean()); }
  torch::Tensor norm_var() { return norm_state(s_->norm_var()); }
  torch::Tensor norm_gain() { return norm_state(s_->norm_gain()); }

  void reset() { s_->reset(); }
  int64_t d_max() const { return (int64_t)s_->d_max(); }
  int64_t rows() const { return (int64_t)s_->rows(); }
  int64_t channels() const { return (int64_t)s_->channels(); }
  int64_t trials() const { return (int64_t)s_->trials(); }

 private:
  template <typename T>
  torch::Tensor norm_state(const T* dev) {
    TORCH_CHECK(s_->normalize(),
                "IncoherentSearch: built without normalize, no state");
    check(hipStreamSynchronize(s_->stream()), "incoherent stream sync");
    auto out = torch::empty(
        {(int64_t)s_->channels()},
        torch::TensorOptions().dtype(c10::CppTypeToScalarType<T>::value));
    check(hipMemcpy(out.data_ptr(), dev, s_->channels() * sizeof(T),
                    hipMemcpyDeviceToHost),
          "incoherent state d2h");
    return out;
  }

  std::unique_ptr<IncoherentSearch> s_;
  hipEvent_t ev_ = nullptr;
};

}  // namespace

PYBIND11_MODULE(TORCH_EXTENSION_NAME, m) {
  m.doc() = "srtb_amd MI355X-native kernels + pipeline engine";
  m.def("unpack", &t_unpack, py::arg("raw"), py::arg("nbits"),
        py::arg("out_count"), py::arg("window") = c10::nullopt);
  m.def("unpack_2pol", &t_unpack_2pol, py::arg("raw"), py::arg("kind"),
        py::arg("window") = c10::nullopt);
  m.def("unpack_gznupsr_a1", &t_unpack_gznupsr, py::arg("raw"),
        py::arg("n_streams"), py::arg("window") = c10::nullopt);
  m.def("build_window", &t_build_window, py::arg("n"), py::arg("kind"),
        py::arg("device") = torch::Device(torch::kCUDA));
  m.def("mean_power", &t_mean_power, py::arg("spec"), py::arg("blocks") = 0);
  m.def("sum_sumsq", &t_sum_sumsq);
  m.def("rfi_s1", &t_rfi_s1);
  m.def("zap_bins", &t_zap_bins);
  m.def("dedisperse", &t_dedisperse);
  m.def("dedisp_phase_table", &t_phase_table);
  m.def("rfi_dedisperse_fused", &t_rfi_dedisperse_fused, py::arg("spec"),
        py::arg("enable_rfi"), py::arg("threshold"), py::arg("channel_count"),
        py::arg("ranges"), py::arg("f_min"), py::arg("f_c"), py::arg("df"),
        py::arg("dm"), py::arg("table") = c10::nullopt,
        py::arg("out") = c10::nullopt);
  m.def("detect_peaks", &t_detect_peaks, py::arg("ts"), py::arg("cumsum"),
        py::arg("lengths"));
  m.def("sk_row_stats", &t_sk_row_stats);
  m.def("sk_mitigate", &t_sk_mitigate);
  m.def("sk_v1_mitigate", &t_sk_v1_mitigate, py::arg("wf"),
        py::arg("sk_threshold"), py::arg("normalize") = false);
  m.def("time_series", &t_time_series, py::arg("wf"), py::arg("flags"),
        py::arg("ts_count"));
  m.def("subtract_mean", &t_subtract_mean);
  m.def("count_signal", &t_count_signal);
  m.def("inclusive_scan", &t_inclusive_scan);
  m.def("boxcar", &t_boxcar);
  m.def("boxcar_ladder", &t_boxcar_ladder, py::arg("cumsum"),
        py::arg("lengths"), py::arg("snr"));
  m.def("resample_power", &t_resample_power);
  m.def("normalize_by_mean", &t_normalize_by_mean);
  m.def("generate_pixmap", &t_generate_pixmap);
  m.def("running_mean", &t_running_mean);
  m.def("correlate", &t_correlate, py::arg("f1"), py::arg("f2"),
        py::arg("scale"), py::arg("out") = py::none());
  m.def("complex_abs", &t_complex_abs, py::arg("x"));
  m.def("filterbank_detect", &t_filterbank_detect, py::arg("wf"),
        py::arg("flags"), py::arg("valid_rows"), py::arg("tscrunch"),
        py::arg("fscrunch"), py::arg("reverse"));
  m.def("filterbank_detect_pol", &t_filterbank_detect_pol, py::arg("wf_a"),
        py::arg("wf_b"), py::arg("flags_a"), py::arg("flags_b"),
        py::arg("valid_rows"), py::arg("tscrunch"), py::arg("fscrunch"),
        py::arg("reverse"), py::arg("pol_state"));
  m.def("filterbank_channel_stats", &t_filterbank_channel_stats, py::arg("P"));
  m.def("filterbank_quantize", &t_filterbank_quantize, py::arg("P"),
        py::arg("mean"), py::arg("std"));
  m.def("fold_block", &t_fold_block, py::arg("wf"), py::arg("flags"),
        py::arg("valid"), py::arg("nbin"), py::arg("phi"), py::arg("dphi"),
        py::arg("acc"), py::arg("hits"), py::arg("weights"));
  m.def("native_fft", &t_native_fft, py::arg("x"), py::arg("sign"));
  m.def("native_fft_sk", &t_native_fft_sk, py::arg("x"));
  m.def("native_rfft", &t_native_rfft, py::arg("x"));
  m.def("native_rfft_raw", &t_native_rfft_raw, py::arg("raw"),
        py::arg("nbits"));
  m.def("native_rfft_final_partials", &t_native_rfft_final_partials,
        py::arg("n"));
  m.def("preop_backward_fft", &t_preop_backward_fft, py::arg("spec"),
        py::arg("maxcol_log2"), py::arg("final_log2"), py::arg("f_min"),
        py::arg("f_c"), py::arg("df"), py::arg("dms"),
        py::arg("ranges") = std::vector<std::vector<int64_t>>{},
        py::arg("enable_rfi") = false, py::arg("threshold") = 0.0,
        py::arg("channel_count") = 1);
  m.def("dedisp_poly_factors", &t_dedisp_poly_factors);
  m.def("bench_fft", &t_bench_fft, py::arg("len"), py::arg("batch"),
        py::arg("sign"), py::arg("iters") = 20, py::arg("backend") = "native");
  m.def("bench_rfft", &t_bench_rfft, py::arg("n"), py::arg("iters") = 20,
        py::arg("backend") = "native");

  py::class_<PyEngine>(m, "PipelineEngine")
      .def(py::init<int64_t, int64_t, int64_t, double, double, double, double,
                    double, double, double, int64_t, int64_t,
                    std::vector<std::vector<int64_t>>, bool, bool, bool,
                    int64_t, int64_t, int64_t, bool, int64_t, int64_t,
                    int64_t, int64_t, int64_t, double, double, double>(),
           py::arg("n"), py::arg("nbits"), py::arg("channels"),
           py::arg("freq_low"), py::arg("bandwidth"), py::arg("sample_rate"),
           py::arg("dm"), py::arg("rfi_threshold") = 10.0,
           py::arg("sk_threshold") = 1.1, py::arg("snr_threshold") = 6.0,
           py::arg("max_boxcar") = 1024, py::arg("nsamps_reserved") = 0,
           py::arg("zap_ranges") = std::vector<std::vector<int64_t>>{},
           py::arg("use_phase_table") = false,
           py::arg("enable_rfi_s1") = true, py::arg("enable_sk") = true,
           py::arg("n_slots") = 2, py::arg("fft_backend") = 2,
           py::arg("window_kind") = 0, py::arg("use_hip_graph") = false,
           py::arg("max_dm_trials") = 0, py::arg("fil_tscrunch") = 0,
           py::arg("fil_fscrunch") = 1, py::arg("fil_nbits") = 32,
           py::arg("fold_nbin") = 0, py::arg("fold_f0") = 0.0,
           py::arg("fold_f1") = 0.0, py::arg("fold_phase0") = 0.0)
      .def("submit", &PyEngine::submit, py::arg("raw"),
           py::arg("dm_override") = std::nan(""))
      .def("submit_samples", &PyEngine::submit_samples, py::arg("samples"),
           py::arg("dm_override") = std::nan(""))
      .def("wait", &PyEngine::wait)
      .def("submit_trials", &PyEngine::submit_trials, py::arg("raw"),
           py::arg("dms"))
      .def("submit_trials_samples", &PyEngine::submit_trials_samples,
           py::arg("samples"), py::arg("dms"))
      .def("wait_trials", &PyEngine::wait_trials)
      .def("select_trial", &PyEngine::select_trial)
      .def("dm_time_plane", &PyEngine::dm_time_plane)
      .def("cumsum", &PyEngine::cumsum)
      .def("synchronize", &PyEngine::synchronize)
      .def("waterfall", &PyEngine::waterfall, py::arg("slot"),
           py::arg("zap") = true)
      .def("sk_stats", &PyEngine::sk_stats)
      .def("sk_flags", &PyEngine::sk_flags)
      .def("time_series", &PyEngine::time_series)
      .def("boxcar_series", &PyEngine::boxcar_series)
      .def("filterbank", &PyEngine::filterbank)
      .def("filterbank_power", &PyEngine::filterbank_power)
      .def("filterbank_stats", &PyEngine::filterbank_stats)
      .def("set_fold_next_sample", &PyEngine::set_fold_next_sample)
      .def("fold_next_sample", &PyEngine::fold_next_sample)
      .def("fold_words", &PyEngine::fold_words)
      .def("fold_reset", &PyEngine::fold_reset)
      .def("fold_read", &PyEngine::fold_read)
      .def_property_readonly("filterbank_rows", &PyEngine::filterbank_rows)
      .def_property_readonly("filterbank_channels",
                             &PyEngine::filterbank_channels)
      .def_property_readonly("n", &PyEngine::n)
      .def_property_readonly("nc", &PyEngine::nc)
      .def_property_readonly("n_channels", &PyEngine::n_channels)
      .def_property_readonly("waterfall_len", &PyEngine::waterfall_len)
      .def_property_readonly("ts_count", &PyEngine::ts_count)
      .def_property_readonly("raw_bytes", &PyEngine::raw_bytes)
      .def_property_readonly("n_slots", &PyEngine::n_slots);

  py::class_<PyPolCombiner>(m, "PolCombiner")
      .def(py::init<int64_t, int64_t, int64_t, int64_t, int64_t, bool,
                    int64_t, int64_t, int64_t>(),
           py::arg("n"), py::arg("channels"), py::arg("nsamps_reserved") = 0,
           py::arg("tscrunch") = 16, py::arg("fscrunch") = 1,
           py::arg("reverse") = false, py::arg("pol_state") = 2,
           py::arg("nbits") = 32, py::arg("n_slots") = 2)
      .def("submit", &PyPolCombiner::submit, py::arg("eng_a"),
           py::arg("slot_a"), py::arg("eng_b"), py::arg("slot_b"))
      .def("wait", &PyPolCombiner::wait)
      .def("plane", &PyPolCombiner::plane)
      .def("power", &PyPolCombiner::power)
      .def("stats", &PyPolCombiner::stats)
      .def_property_readonly("rows", &PyPolCombiner::rows)
      .def_property_readonly("channels", &PyPolCombiner::channels)
      .def_property_readonly("nifs", &PyPolCombiner::nifs);

  m.def("incoh_dedisperse", &t_incoh_dedisperse, py::arg("window"),
        py::arg("delays"), py::arg("R"));
  m.def("incoh_detect", &t_incoh_detect, py::arg("Y"), py::arg("snr"),
        py::arg("max_boxcar"));
  m.def("incoh_norm_update", &t_incoh_norm_update, py::arg("plane"),
        py::arg("alpha"), py::arg("M"), py::arg("V"), py::arg("G"));
  m.def("incoh_norm_apply", &t_incoh_norm_apply, py::arg("plane"),
        py::arg("M"), py::arg("G"), py::arg("ring"), py::arg("write_row"));
  m.attr("INCOH_CHANNEL_CHUNK") = (int64_t)kIncohChannelChunk;
  m.attr("INCOH_MAX_ROWS") = (int64_t)kIncohMaxRows;
  py::class_<PyIncoherentSearch>(m, "IncoherentSearch")
      .def(py::init<int64_t, int64_t, double, double, double,
                    std::vector<double>, double, int64_t, int64_t, bool,
                    int64_t>(),
           py::arg("rows"), py::arg("channels"), py::arg("fch1"),
           py::arg("foff"), py::arg("tsamp"), py::arg("offsets"),
           py::arg("snr_threshold"), py::arg("max_boxcar"),
           py::arg("n_slots") = 2, py::arg("normalize") = false,
           py::arg("normalize_blocks") = 8)
      .def("submit", &PyIncoherentSearch::submit, py::arg("engine"),
           py::arg("slot"))
      .def("submit_plane", &PyIncoherentSearch::submit_plane, py::arg("plane"))
      .def("wait", &PyIncoherentSearch::wait)
      .def("plane", &PyIncoherentSearch::plane)
      .def("delays", &PyIncoherentSearch::delays)
      .def("reset", &PyIncoherentSearch::reset)
      .def("norm_mean", &PyIncoherentSearch::norm_mean)
      .def("norm_var", &PyIncoherentSearch::norm_var)
      .def("norm_gain", &PyIncoherentSearch::norm_gain)
      .def_property_readonly("d_max", &PyIncoherentSearch::d_max)
      .def_property_readonly("rows", &PyIncoherentSearch::rows)
      .def_property_readonly("channels", &PyIncoherentSearch::channels)
      .def_property_readonly("trials", &PyIncoherentSearch::trials);
}
