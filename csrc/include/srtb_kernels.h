// srtb_amd — MI355X-native kernel API (CDNA4 / gfx950, wave64).
//
// Raw-pointer + hipStream_t interface so the same kernels serve the torch
// extension, the native engine, and the standalone tools.  Each function
// enqueues asynchronously on the given stream and returns the first HIP error.
//
// Semantics mirror the reference pipeline (citations per kernel in the .hip
// files); the implementations are designed for gfx950: 64-wide wavefronts,
// vectorized (float4 / uint4) global access, grid-stride loops capped per
// CDNA guideline G11, two-pass deterministic reductions with fp64 partials.

#pragma once

#include <hip/hip_runtime.h>
#include <cstddef>
#include <cstdint>

namespace srtb_hip {

// ---------------- unpack (reference unpack.hpp:43-403) ----------------
// nbits: 1, 2, 4 = unsigned MSB-first packed; 8/-8, 16/-16, 32/-32 = u/int
// cast.  window (nullable) multiplies out[i] by window[i] (fused FFT window).
//
// Counts.  A launcher covers exactly the count it is given or returns
// hipErrorInvalidValue and launches nothing; it never drops a remainder:
//  - unpack, 1/2/4 bits: out_count * nbits must be a multiple of 8 (whole
//    input bytes); any number of bytes is covered.
//  - unpack, 8/-8 bits: any out_count (whole 4-sample words, then the
//    out_count % 4 samples after them bytewise); 16/32 bits: any out_count.
//  - two-pol, SNAP-1 and GZNU: the count per polarization / per stream must be
//    a multiple of 4 (one lane decodes 4 samples of every stream).
// Alignment assumed, not checked: `in` 4-byte aligned for the sub-byte and
// 8-bit paths (dword loads), element-aligned for the 16/32-bit casts, 8-byte
// aligned for two-pol and SNAP-1 (uint2 loads), 4-byte aligned for GZNU;
// every output 16-byte aligned (float4 stores); window as float.
hipError_t unpack(const uint8_t* in, float* out, size_t out_count, int nbits,
                  const float* window, hipStream_t stream);

// int8 samples interleaved per-sample: p0 s0, p1 s0, p0 s1, ...
hipError_t unpack_interleaved_2pol(const int8_t* in, float* out0, float* out1,
                                   size_t count_per_pol, const float* window,
                                   hipStream_t stream);

// SNAP-1 "1 1 2 2": groups of 4 int8 = [s0p0 s1p0 s0p1 s1p1]
hipError_t unpack_naocpsr_snap1(const int8_t* in, float* out0, float* out1,
                                size_t count_per_pol, const float* window,
                                hipStream_t stream);

// GZNU A1: 4-byte words cycling over n_streams (2 or 4) ADCs; 4-stream
// variant is offset-binary (^0x80).  outs[s] may be null for unused streams.
hipError_t unpack_gznupsr_a1(const uint8_t* in, float* out0, float* out1,
                             float* out2, float* out3, int n_streams,
                             size_t count_per_stream, const float* window,
                             hipStream_t stream);

// FFT window coefficient table (0 = rectangle [no-op values], 1 = hann,
// 2 = hamming) — reference fft/fft_window.hpp.
hipError_t build_window(float* coef, size_t n, int kind, hipStream_t stream);

// ---------------- reductions ----------------
// Deterministic two-pass mean of |x|^2 over n complex bins.
// partials: device scratch of n_partials doubles (n_partials = reduce grid),
// out: 1 double = mean.  Use reduce_partials() to size the scratch.
int reduce_partials();  // number of fp64 partials the reductions use

// blocks: pass-1 grid, 1 .. reduce_partials() / 2; 0 = the default of 1024
// (every production call).  Pass 2 sums exactly the partials pass 1 wrote.
// A smaller grid is the test surface for the per-thread fp64 drain, which a
// thread reaches after 1024 trips of its loop (2^19 bins at blocks = 1).
hipError_t mean_power(const float2* in, size_t n, double* partials,
                      double* out_mean, hipStream_t stream, int blocks = 0);

// sum and sum-of-squares over a float array (two outputs in one pass):
// out[0] = sum, out[1] = sum of squares
hipError_t sum_sumsq(const float* in, size_t n, double* partials,
                     double* out2, hipStream_t stream);

// ---------------- RFI stage 1 + coherent dedispersion ----------------
// Standalone RFI s1: zap |x|^2 > threshold*mean, else scale by norm_coeff
// (reference rfi_mitigation_pipe.hpp:50-80).  mean is a device scalar.
hipError_t rfi_s1(float2* spec, size_t n, const double* mean_power,
                  float threshold, float norm_coeff, hipStream_t stream);

// Manual zap of inclusive bin range (reference rfi_mitigation.hpp:97-157).
// hi < lo returns hipErrorInvalidValue; the launcher does not know the
// spectrum's length, so hi < length is the caller's to check.
hipError_t zap_bins(float2* spec, size_t lo, size_t hi, hipStream_t stream);

// Standalone coherent dedispersion, fp64 phase (reference
// coherent_dedispersion.hpp:133-248): x[i] *= exp(-2pi*i*frac(k)),
// k = D*1e6*dm/f*((f-f_c)/f_c)^2, f = f_min + df*i.
hipError_t dedisperse(float2* spec, size_t n, double f_min, double f_c,
                      double df, double dm, hipStream_t stream);

// Precompute the per-bin phase-factor table (table mode for fixed DM).
hipError_t dedisp_phase_table(float2* table, size_t n, double f_min,
                              double f_c, double df, double dm,
                              hipStream_t stream);

// Fused hot-path kernel: RFI-s1 zap + normalize + manual zap ranges +
// dedispersion phase rotation in ONE pass over the spectrum (the reference
// runs three separate kernels + waits; fusing removes two full HBM
// round-trips of the 4 GB spectrum).  zap_ranges: up to 16 inclusive [lo,hi]
// bin pairs, read from constant args.  factor_table: optional precomputed
// phases (else computed on the fly in fp64).
struct ZapRange { unsigned long long lo, hi; };
hipError_t rfi_dedisperse_fused(float2* spec, size_t n,
                                const double* mean_power, float threshold,
                                float norm_coeff, const ZapRange* ranges,
                                int n_ranges, double f_min, double f_c,
                                double df, double dm,
                                const float2* factor_table,
                                hipStream_t stream);
// Out-of-place form: reads `in`, writes every bin of `out`; `in` is never
// written (the DM-trial path keeps it as the block's forward spectrum).
// out == in is the in-place kernel above; otherwise the two buffers must not
// overlap.
hipError_t rfi_dedisperse_fused(const float2* in, float2* out, size_t n,
                                const double* mean_power, float threshold,
                                float norm_coeff, const ZapRange* ranges,
                                int n_ranges, double f_min, double f_c,
                                double df, double dm,
                                const float2* factor_table,
                                hipStream_t stream);

// ---------------- spectral kurtosis (stage 2) ----------------
// Per-row <sum |x|^2, sum |x|^4> of a [rows][len] waterfall; one workgroup
// per row (reference multi_mapreduce + rfi_mitigation.hpp:310-340).
hipError_t sk_row_stats(const float2* wf, size_t rows, size_t len,
                        float2* s2s4, hipStream_t stream);

// Decide zap flags from SK statistic: flag[i] = SK outside [lo_, hi_]
// (corrected thresholds precomputed on host), and count rows whose first
// sample is zero OR flagged (the reference's zapped-channel count observes
// column 0 after zapping).  zero_count must be zeroed beforehand.
hipError_t sk_flags(const float2* wf, const float2* s2s4, size_t rows,
                    size_t len, float lo_corrected, float hi_corrected,
                    uint8_t* flags, unsigned* zero_count, hipStream_t stream);

// wave-local small FFT: n in {256,512,1024}, one FFT per wave (batched,
// contiguous); tw_n = n-entry twiddle table with the sign baked in
hipError_t fft_wave_pass(const float2* in, float2* out, uint32_t n,
                         size_t n_ffts, int sign, const float2* tw_n,
                         hipStream_t stream);

// K21: waterfall window de-apply — wf[i] /= coef[i mod len] (reference
// fft_pipe.hpp:350-358; only for non-rectangle FFT windows)
hipError_t window_deapply(float2* wf, const float* coef, size_t total,
                          size_t len, hipStream_t stream);

// Zero out flagged rows.
hipError_t sk_zap_rows(float2* wf, const uint8_t* flags, size_t rows,
                       size_t len, hipStream_t stream);

// SK method 1 (reference rfi_mitigation.hpp:183-274): time-major [M][bins]
// waterfall; thresholds already corrected like sk_flags.  normalize applies
// the optional per-bin 1/sqrt(mean|x|^2) of surviving bins.
hipError_t sk_v1_stats(const float2* wf, size_t M, size_t bins, float2* s2s4,
                       hipStream_t stream);
hipError_t sk_v1_zap(float2* wf, size_t M, size_t bins, const float2* s2s4,
                     float lo_corrected, float hi_corrected, bool normalize,
                     hipStream_t stream);

// ---------------- signal detection ----------------
// ts[j] = sum_i |wf[i][j]|^2 over non-flagged rows, j < ts_count
// (reference signal_detect_pipe.hpp:305-316; flags may be null).
hipError_t time_series(const float2* wf, const uint8_t* flags, size_t rows,
                       size_t len, size_t ts_count, float* ts,
                       hipStream_t stream);

// Two-stage variant for large shapes: partial must hold
// time_series_chunks(ts_count) * ts_count floats; deterministic, ~10x the
// bandwidth of the single-pass kernel at S=2048, L=64k.
int time_series_chunks(size_t ts_count);
hipError_t time_series_2stage(const float2* wf, const uint8_t* flags,
                              size_t rows, size_t len, size_t ts_count,
                              float* ts, float* partial, hipStream_t stream);

// ts[i] -= sum/n (baseline subtract; sum is a device scalar from sum_sumsq).
hipError_t subtract_mean(float* ts, size_t n, const double* sum,
                         hipStream_t stream);

// threshold = snr * sqrt(sumsq/n) (device scalar sumsq of the zero-mean
// series); appends count of ts[i] > threshold into out_count (atomic; zero it
// first) and writes the threshold to out_threshold (reference
// signal_detect.hpp:33-67).
hipError_t count_above(const float* ts, size_t n, const double* sumsq,
                       float snr, unsigned* out_count, float* out_threshold,
                       hipStream_t stream);

// Inclusive prefix sum (float in → float out); scratch must hold
// scan_scratch_size(n) floats (one per 2048-element block).
int scan_scratch_size(size_t n);
hipError_t inclusive_scan(const float* in, float* out, size_t n,
                          float* scratch, hipStream_t stream);

// box[i] = cumsum[i+L] - cumsum[i], i < n_out (reference
// signal_detect_pipe.hpp:387-423).
// fused boxcar ladder: thresholds + counts for up to 12 lengths in 3
// launches, derived directly from the cumulative sum (no box arrays).
// partials: device scratch of n_lengths * 2 * reduce_partials() doubles;
// out_thr/out_counts: [n_lengths] each (counts must be zeroed beforehand).
// A length >= ts_count has no window: its count stays 0 and its threshold
// carries no meaning (0, or NaN for a length equal to ts_count); the engine
// never builds such a ladder.
hipError_t boxcar_ladder(const float* cumsum, size_t ts_count,
                         const size_t* lengths, int n_lengths,
                         double* partials, float snr, float* out_thr,
                         unsigned* out_counts, hipStream_t stream);

hipError_t boxcar(const float* cumsum, float* out, size_t n_out, size_t L,
                  hipStream_t stream);

// Peaks of the raw series and of every ladder length in one pass:
//   out_value[0], out_index[0]     = max ts[i] and the lowest i attaining it
//   out_value[1+l], out_index[1+l] = the same over cumsum[i+L_l] - cumsum[i],
//                                    i + L_l < ts_count (boxcar's indexing)
// Deterministic and independent of the launch geometry.  A length with no
// valid window reports -infinity at index UINT_MAX.  scratch: device memory
// of detect_peaks_scratch_bytes(), no initialization needed.  cumsum may be
// null when n_lengths == 0; n_lengths <= 12, ts_count < 2^32.
size_t detect_peaks_scratch_bytes();
hipError_t detect_peaks(const float* ts, const float* cumsum, size_t ts_count,
                        const size_t* lengths, int n_lengths, void* scratch,
                        float* out_value, unsigned* out_index,
                        hipStream_t stream);

// ---------------- filterbank output (csrc/kernels/filterbank.hip) ----------
// Definition: docs/ARCHITECTURE.md, "Filterbank output".
constexpr size_t kFilterbankMaxTscrunch = 4096;
constexpr int kFilterbankQuantLevel = 64;     // 8-bit level of the mean
constexpr int kFilterbankQuantPerSigma = 16;  // 8-bit levels per sigma

// out[r][c] (R = V / tscrunch rows, C = S / fscrunch channels, c fastest) =
// sum of |wf[row][t]|^2 over the cell's fscrunch waterfall rows and tscrunch
// time samples, taken from the first V columns of the [S][L] waterfall.
// Output channel c holds rows c*fscrunch ... (reverse = false) or
// S-(c+1)*fscrunch ... (reverse = true).  Rows with flags[row] != 0
// contribute 0; flags may be null.  One pass, no atomics, bit-identical from
// run to run.  tscrunch: power of two <= kFilterbankMaxTscrunch, fscrunch
// divides S, tscrunch <= V <= L, L even (rows are read as float4).
hipError_t filterbank_detect(const float2* wf, const uint8_t* flags, size_t S,
                             size_t L, size_t V, size_t tscrunch,
                             size_t fscrunch, bool reverse, float* out,
                             hipStream_t stream);

// Polarization products of two waterfalls of the same sky (definition:
// docs/ARCHITECTURE.md, "Polarization products").  With A = x+iy = wf_a and
// B = u+iv = wf_b at the same row and column: AA = x^2+y^2, BB = u^2+v^2,
// CR = xu+yv, CI = yu-xv, each summed over the cell exactly as
// filterbank_detect sums its power.  out[r][p][c] ([R][P][C], c fastest):
// pol_state I -> P = 1: AA+BB; AABBCRCI -> P = 4: AA, BB, CR, CI; IQUV ->
// P = 4: AA+BB, AA-BB, 2CR, 2CI, formed from the four fp32 cell sums.  A row
// flagged in either flags_a or flags_b contributes 0 to every product; either
// pointer may be null.  wf_a, wf_b: [S][L] each, 16-byte aligned; out:
// R * P * C floats; flags: [S] bytes.  One pass, no atomics, bit-identical
// from run to run.  Geometry rules of filterbank_detect; anything else, or a
// pol_state outside the three, returns hipErrorInvalidValue.
constexpr int kPolStateI = 0;
constexpr int kPolStateAABBCRCI = 1;
constexpr int kPolStateIQUV = 2;
int pol_state_nifs(int pol_state);  // P: 1 or 4; 0 = not a state
hipError_t filterbank_detect_pol(const float2* wf_a, const float2* wf_b,
                                 const uint8_t* flags_a,
                                 const uint8_t* flags_b, size_t S, size_t L,
                                 size_t V, size_t tscrunch, size_t fscrunch,
                                 bool reverse, int pol_state, float* out,
                                 hipStream_t stream);

// Per-channel mean and (population) standard deviation of P[R][C], two-stage
// with fp64 partials combined in fixed order, stored as float.  partials:
// device scratch of filterbank_stats_partials(C) doubles.
size_t filterbank_stats_partials(size_t C);
hipError_t filterbank_channel_stats(const float* P, size_t R, size_t C,
                                    double* partials, float* mean,
                                    float* stddev, hipStream_t stream);

// out[r][c] = clamp(rint((P - mean_c) * (16 / std_c) + 64), 0, 255) in fp32;
// 64 where std_c = 0.
hipError_t filterbank_quantize(const float* P, const float* mean,
                               const float* stddev, size_t R, size_t C,
                               uint8_t* out_u8, hipStream_t stream);

// ---------------- pulsar folding (csrc/kernels/fold.hip) ----------------
// Definition: docs/ARCHITECTURE.md, "Pulsar folding".
constexpr size_t kFoldMinBins = 2;
constexpr size_t kFoldMaxBins = 65536;

// Folds the first V columns of the [S][L] waterfall at the phase words
// words[0] = Phi, words[1] = dPhi (device memory, wrapping 64-bit fixed
// point, 2^64 = one turn): column k has bin
// (((Phi + k * dPhi) >> 32) * nbin) >> 32, and
//   acc[c][b]  += sum of |wf[c][k]|^2 over the columns of bin b (fp64 [S][nbin])
//   hits[b]    += number of columns of bin b
//   weights[c] += V
// where a row with flags[c] != 0 adds nothing to acc and weights; flags may
// be null.  Every element is read, added to and written by one thread: no
// atomics, bit-identical from run to run.  table: device scratch of
// fold_table_words(V) 32-bit words.  1 <= V <= L, V < 2^31,
// kFoldMinBins <= nbin <= kFoldMaxBins.
size_t fold_table_words(size_t V);
hipError_t fold_block(const float2* wf, const uint8_t* flags, size_t S,
                      size_t L, size_t V, size_t nbin, const uint64_t* words,
                      uint32_t* table, double* acc, uint64_t* hits,
                      uint64_t* weights, hipStream_t stream);

// ---------------- incoherent DM-offset search (csrc/kernels/incoherent.hip) --
// Definition: docs/ARCHITECTURE.md, "Incoherent DM-offset search".
constexpr size_t kIncohMaxTrials = 1024;
constexpr size_t kIncohMinRows = 2;
// incoh_detect keeps a trial's fp64 scan in LDS, one workgroup per trial:
// 16384 rows * 8 bytes = 128 KiB of the 160 KiB of a gfx950 CU
constexpr size_t kIncohMaxRows = 16384;
constexpr size_t kIncohMaxDelay = (size_t)1 << 20;  // D_max, rows
// (D_max + R) * C * 4 bytes of history; 1 GiB is 64 full-size planes
// (R = 16384, C = 4096) and far below what the engine itself allocates
constexpr size_t kIncohMaxWindowBytes = (size_t)1 << 30;
constexpr size_t kIncohChannelChunk = 1024;  // channels per partial sum
constexpr int kIncohMaxLengths = 21;  // boxcar lengths 1, 2, 4 ... 2^20

// Y[t][j] = sum_c W[j + delays[t][c]][c] in fp32, t < T, j < R, where row w
// of the window W is row (row0 + w) mod ring_rows of `window`
// ([ring_rows][C] floats, ring_rows >= R; a linear window is row0 = 0).
// delays: [T][C] int32 with every entry in 0 .. ring_rows - R, which the
// caller guarantees (the kernel does not check).  Channels are summed in
// chunks of kIncohChannelChunk; with more than one chunk, `partials` must hold
// incoh_partials(T, R, C) floats (else it may be null).  The order of
// summation depends on C and the launch constants only; no atomics,
// bit-identical from run to run.  Geometry outside the limits above returns
// hipErrorInvalidValue and launches nothing.
int incoh_chunks(size_t C);
size_t incoh_partials(size_t T, size_t R, size_t C);
hipError_t incoh_dedisperse(const float* window, size_t ring_rows, size_t row0,
                            const int* delays, size_t T, size_t R, size_t C,
                            float* partials, float* Y, hipStream_t stream);

// Detection on every row of Y[T][R] in one launch, fp64 throughout, for the
// n_lengths boxcar lengths 1, 2, 4 ... (incoh_lengths(max_boxcar) of them):
// mu[t] = mean of the row, z = Y - mu, cs = inclusive scan of z; length 1 is
// z itself (n = R values), length l >= 2 is cs[i + l] - cs[i], i + l < R.
// Per (t, length), [T][n_lengths]: peak and the lowest index attaining it,
// rms = sqrt(sum b^2 / n), count = #{b > snr * rms}.  A length >= R has no
// window: peak -infinity, index UINT_MAX, rms 0, count 0.
// kIncohMinRows <= R <= kIncohMaxRows.
int incoh_lengths(size_t max_boxcar);
hipError_t incoh_detect(const float* Y, size_t T, size_t R, int n_lengths,
                        double snr, double* out_peak, unsigned* out_index,
                        double* out_rms, unsigned* out_count, double* out_mu,
                        hipStream_t stream);

// Per-channel normalisation of a block before it enters the history
// (docs/ARCHITECTURE.md, "Per-channel normalisation").
constexpr size_t kIncohNormMaxBlocks = 65536;  // K of the running average

// Block statistics of plane[R][C] and one step of the running state, all
// fp64: with x0 = plane[0][c], s = sum_r (x - x0), s2 = sum_r (x - x0)^2
// (row chunks summed in chunk order, a fixed number of them),
//   m = x0 + s / R,   v = max(s2 / R - (s / R)^2, 0)
//   M[c] += alpha * (m - M[c]),   V[c] += alpha * (v - V[c])
// every operation rounded on its own, then G[c] = (float)(1 / sqrt(V[c]))
// where V[c] > 0, else 0, and *live = #{c : G[c] > 0}.  M, V, G are updated in
// place.  partials: device scratch of incoh_norm_partials(C) doubles.  The
// order of summation depends on R, C and launch constants only; no atomics.
// R == 0, C == 0 or a null pointer returns hipErrorInvalidValue and launches
// nothing.
size_t incoh_norm_partials(size_t C);
hipError_t incoh_norm_update(const float* plane, size_t R, size_t C,
                             double alpha, double* partials, double* M,
                             double* V, float* G, unsigned* live,
                             hipStream_t stream);

// ring[(write_row + r) mod ring_rows][c] = (plane[r][c] - (float)M[c]) * G[c],
// r < R: one fp32 subtraction and one fp32 multiplication, each rounded on its
// own.  16-byte accesses where C % 4 == 0 and plane, ring and G are 16-byte
// aligned, scalar ones otherwise, with the same bits.  The other ring rows are
// not touched.  R == 0, C == 0, ring_rows < R, write_row >= ring_rows or a
// null pointer returns hipErrorInvalidValue and launches nothing.
hipError_t incoh_norm_apply(const float* plane, size_t R, size_t C,
                            const double* M, const float* G, float* ring,
                            size_t ring_rows, size_t write_row,
                            hipStream_t stream);

// ---------------- hand-written Stockham FFT ----------------
// One generic pass of the LDS-staged Stockham FFT (csrc/kernels/fft.hip).
// Index-math oracle: srtb_amd/fftref.py.  Host-side planning:
// csrc/fft/native_fft.h.
struct FftPassDesc {
  uint32_t n;            // pow2 FFT length of this pass (<= 4096)
  uint32_t d0 = 1, d1 = 1;  // instance id -> digits q0, q1, q2 (pow2;
                            // d0 == 0 means "q0 = id" for contiguous rows)
  unsigned long long in_c0 = 0, in_c1 = 0, in_c2 = 0;
  unsigned long long in_stride = 1;
  unsigned long long out_c0 = 0, out_c1 = 0, out_c2 = 0;
  unsigned long long out_stride = 1;
  unsigned long long tw_f0 = 0, tw_f1 = 0;
  unsigned long long tw_mod = 0;  // 0 = no inter-pass twiddle
  int tw_lo_bits = 0;
  double tw_angle = 0.0;  // sign * 2*pi / tw_mod (for computed twiddles)
};

// build table[j] = exp(sign * 2*pi*i * j / m), j in [0, count)
hipError_t fft_build_twiddle(float2* table, size_t count, double m, int sign,
                             hipStream_t stream);

// tw_n: FULL-circle per-length table (n entries, staged into LDS)
hipError_t fft_stockham_pass(const float2* in, float2* out,
                             const FftPassDesc& d, size_t n_ffts, int F,
                             bool load_ffast, bool store_ffast, int sign,
                             const float2* tw_n, const float2* tw_hi,
                             const float2* tw_lo, hipStream_t stream);

// Optional per-element pre-op fused into a column pass's LOADS: the full
// RFI-s1 zap + normalize + manual zap + coherent dedispersion of
// rfi_dedisperse_fused, applied at the element's flat spectrum index
// (= its load address offset).  Fusing it into the backward FFT's first
// pass saves a whole read+write of the 4 GB spectrum per block.
struct FftPreop {
  const double* mean_power = nullptr;  // null = no RFI zap/normalize
  float threshold = 0.f, norm_coeff = 1.f;
  int n_zap = 0;
  ZapRange zap[16] = {};
  double f_min = 0, f_c = 0, df = 0, dm = 0;
  // optional cached dedispersion factors [nc]; when set the pass reads the
  // table (one extra coalesced float2 load) instead of computing the phase.
  // Only of interest where the column-polynomial phase (below) does not
  // apply: that one costs ~10 integer VALU instructions per bin and no
  // extra traffic, whereas the per-bin fp64 formula triples the pass's VALU
  // count and the table adds a 4.3 GB read (measured slower than either)
  const float2* table = nullptr;
  // != 0: the pass input is the PACKED forward spectrum Z (length r2c_m);
  // the r2c pair-combine X[k] = E + w_k O runs at load (eliminates the
  // standalone r2c pass; needs an out-of-place first pass)
  unsigned long long r2c_m = 0;
};

// mean |X|^2 over the r2c spectrum from the PACKED spectrum Z via
// Parseval: sum_{k<m}|X_k|^2 = sum|Z|^2 + (X0^2 - XM^2)/2 with
// X0 = Re Z0 + Im Z0, XM = Re Z0 - Im Z0.  power_partials: per-workgroup
// <sum|Z|^2, _> pairs accumulated by the forward DIF store (the SK-fusion
// machinery), z0 = device pointer to Z[0].
hipError_t r2c_mean_from_power(const float2* power_partials,
                               size_t n_partials, const float2* z0, size_t m,
                               double* out_mean, hipStream_t stream);

// Register-resident column FFT pass (N in {2,4,8,16,32,64}; one FFT per
// thread fully in VGPRs; in-place: out must alias layout of in addressing;
// uses the same FftPassDesc fields; out_* ignored, stores to input layout).
// raw2 (optional): fused unpack (raw_bits in {1, 2, 4, 8, -8, 16, -16}, the
// formats of unpack() above) — the pass loads and decodes raw bytes instead
// of reading `in`: complex element i is real samples (2i, 2i+1).  Requires
// an inter-pass twiddle and no preop; raw2 element-aligned for 16 bits.
hipError_t fft_col_pass(const float2* in, float2* out, const FftPassDesc& d,
                        size_t n_ffts, int sign, const float2* tw_n,
                        const float2* tw_hi, const float2* tw_lo,
                        hipStream_t stream, const FftPreop* preop = nullptr,
                        const uint8_t* raw2 = nullptr, int raw_bits = 2);

// Whether fft_col_pass evaluates this pre-op's dedispersion phase as a
// per-column cubic in wrapping fixed point (csrc/kernels/common.h) instead
// of the per-bin fp64 formula.  True when the cubic's truncation bound
//   D*1e6*|dm| / f^5 * (df*stride*(n-1))^4   (f = smallest |f| of the band)
// is <= 2^-28 turns for THIS dm, no table / r2c mode is set, the pass is the
// backward (sign > 0) twiddled one, and SRTB_DEDISP_POLY is not 0.
bool fft_col_preop_uses_poly(const FftPassDesc& d, size_t n_ffts, int sign,
                             const FftPreop& preop);

// Test surface: out[b] = the factor the polynomial pre-op applies at bin b
// of an nc-bin spectrum laid out as columns of (n, stride), n in {2..64}
// pow2, nc a multiple of n*stride.
hipError_t dedisp_poly_factors(float2* out, size_t nc, uint32_t n,
                               size_t stride, double f_min, double f_c,
                               double df, double dm, hipStream_t stream);

// Final composite pass: in-place radix-4 DIF in LDS with base-4
// digit-reversal folded into the store, plus multi-digit output scatter.
// Input must be fully linear (instance blocks contiguous).  n = 4^t.
struct DifFinalDesc {
  uint32_t n;
  unsigned long long out_c2;         // batch-row coefficient
  unsigned long long out_elem_coef;  // output element stride
  int n_prefix = 0;                  // prefix digits, extraction order
  int pf_bits[4] = {0, 0, 0, 0};
  unsigned long long pf_coef[4] = {0, 0, 0, 0};
};
// sk_partials (optional): DifFinalDesc rows own whole batch rows when
// (n_ffts/batch) % F == 0; each workgroup then accumulates <sum|x|^2,
// sum|x|^4> of its stored elements into
// sk_partials[row * wgs_per_row + wg_in_row] (deterministic, no atomics) —
// this replaces the separate 4 GB sk_row_stats read.  wgs_per_row =
// (L/n)/F.
// EXPERIMENTAL strided 512-point LDS middle pass (see fft.hip); reachable
// only via the SRTB_FFT_FACTORS plan override.
hipError_t fft_mid512_pass(const float2* in, float2* out,
                           const FftPassDesc& d, size_t n_ffts, int sign,
                           const float2* tw_n, hipStream_t stream);

hipError_t fft_dif_final(const float2* in, float2* out, const DifFinalDesc& d,
                         size_t n_ffts, int F, int sign, const float2* tw_n,
                         float2* sk_partials, hipStream_t stream);

// Forward final pass of a batch-1 packed-real transform with the r2c
// pair-combine folded into its store: out receives the ordinary r2c
// spectrum X[0..M) (what fft_dif_final followed by r2c_post_process gives,
// bit for bit) and the packed spectrum Z is never written.  F instances per
// side and workgroup (2F rows in LDS); needs out != in, sign -1, a composite
// plan (n_prefix >= 1) and P = n_ffts = M/n >= 2F.
// mean_partials (optional, fft_dif_final_r2c_wgs(n_ffts, F) doubles): also
// writes mean|X|^2 to out_mean, one deterministic partial per workgroup.
int fft_dif_final_r2c_wgs(size_t n_ffts, int F);  // 0: does not apply
hipError_t fft_dif_final_r2c(const float2* in, float2* out,
                             const DifFinalDesc& d, size_t n_ffts, int F,
                             const float2* tw_n, double* mean_partials,
                             double* out_mean, hipStream_t stream);

// combine the DIF-written partials into per-row <S2,S4>
hipError_t sk_combine_partials(const float2* partials, size_t rows,
                               int wgs_per_row, float2* s2s4,
                               hipStream_t stream);

// packed-real R2C finish: Z = C2C(x_even + i*x_odd) of length m -> true
// spectrum X[0..m) (Nyquist dropped).  In-place safe (x may alias z).
// If mean_partials != null (>= 1024 doubles), also writes mean|X|^2 to
// out_mean (fused RFI-s1 statistic).
hipError_t r2c_post_process(const float2* z, float2* x, size_t m,
                            double* mean_partials, double* out_mean,
                            hipStream_t stream);

// ---------------- display / spectrum simplification ----------------
// Area-averaged power resample of [rows][len] complex waterfall to [H][W]
// floats; one workgroup (64 lanes) per output pixel with LDS tree reduce
// (reference resample_spectrum_3, simplify_spectrum.hpp:423-620; wg=64 was
// measured fastest on wave64 GCN — kept for CDNA4).  rows, len, out_h and
// out_w must all be >= 1, else hipErrorInvalidValue and no launch.
hipError_t resample_power_2d(const float2* wf, size_t rows, size_t len,
                             float* out, int out_h, int out_w,
                             hipStream_t stream);

// sum over img (H*W floats) into partials/out via sum_sumsq; then
// img[i] *= 1/(2*mean) with mean = sum/n (reference simplify_spectrum.hpp:627-644).
hipError_t normalize_by_mean(float* img, size_t n, const double* sum,
                             hipStream_t stream);

// intensity [0,1] → ARGB32 lerp color_0..color_1, else overflow color
// (reference simplify_spectrum.hpp:700-731, config.hpp:60-68).
// Rounding rule, shared with srtb_amd.ref.generate_pixmap: each 8-bit channel
// is a + (b - a) * x rounded to the nearest integer, ties away from zero
// (roundf; the reference truncates).  In range means 0 <= x <= 1, so -0.0 is
// in range and NaN, +-inf and anything below 0 or above 1 take the overflow
// colour.
hipError_t generate_pixmap(const float* intensity, uint32_t* out, size_t n,
                           uint32_t color0, uint32_t color1,
                           uint32_t color_overflow, hipStream_t stream);

// ---------------- misc device algorithms ----------------
// Running-mean 1-bit threshold, time-major [nsamp][nchan]
// (reference algorithm/running_mean.hpp:31-77).  1 <= windowsize <= nsamp,
// else hipErrorInvalidValue and no launch (the mirrored tail indexes
// nsamp + i - windowsize).
hipError_t running_mean_init(const float* data, size_t nsamp, size_t nchan,
                             size_t windowsize, float* ave, hipStream_t stream);
hipError_t running_mean(const float* data, size_t nsamp, size_t nchan,
                        uint8_t* out, size_t windowsize, float* ave,
                        hipStream_t stream);

// mag[i] = |x[i]| for complex input (correlator backward-FFT epilogue)
hipError_t complex_abs(const float2* x, float* mag, size_t n,
                       hipStream_t stream);

// correlator pointwise: corr[i] = scale * f1[i]*conj(f2[i]); mag[i] = |corr[i]|
// (reference src/correlator.cpp:116-140; mag may be null).  corr may alias
// f1 or f2 exactly (srtb-correlator writes over f1): every thread reads its
// element of both inputs before it writes.  A partial overlap is not allowed.
hipError_t correlate_pointwise(const float2* f1, const float2* f2,
                               float2* corr, float* mag, size_t n, float scale,
                               hipStream_t stream);

}  // namespace srtb_hip
