// Pulsar folding kernels: the block's coherently dedispersed [S][L] waterfall
// -> per-row pulse profiles acc[S][nbin] (fp64), the bin occupancy hits[nbin]
// and the row weights[S].  Definition: docs/ARCHITECTURE.md, "Pulsar
// folding".  NumPy oracle: srtb_amd.ref.fold_bins / fold_block.
//
// The phase of column k is the wrapping 64-bit word phi_k = Phi + k * dPhi
// (2^64 = one turn), its bin ((phi_k >> 32) * nbin) >> 32.  Within one turn
// the bin never decreases with k, so the samples of one (turn, bin) pair are
// one contiguous run of columns.
//
// MI355X design notes:
//  - fold_turns writes the first column of every turn, at most V + 1 entries
//    whatever nbin and dPhi are.  The run of (turn, bin) then follows without
//    a table: the first column at or above a bin's phase threshold is one
//    fp64 multiply by 1 / dPhi plus an exact integer fix-up of at most a step
//    or two.  Skipped bins (dPhi * nbin > 2^64) are empty runs, dPhi = 0 is
//    one turn whose only non-empty run is the whole block.
//  - fold_accumulate gives a workgroup one row and kBlock adjacent bins.  Per
//    turn those bins own one contiguous span of the row.  The workgroup loads
//    the span with consecutive lanes on consecutive float2 (four independent
//    loads per lane in flight), leaves |.|^2 in LDS, and every thread sums
//    its own run from there in ascending k in fp32.  The LDS stage is double
//    buffered: the next chunk's loads are issued before this one is summed.
//    The runs of a thread are combined in fp64 in turn order and added to acc
//    once, by the only thread that owns that element.  No atomics; the
//    summation order depends only on (V, nbin, Phi, dPhi).
//  - Phi and dPhi are read from device memory, so a captured launch stays
//    valid when the words change from block to block.

#include "common.h"
#include "../include/srtb_kernels.h"

namespace srtb_hip {

namespace {

constexpr int kFoldLoads = 4;                     // float2 per lane and chunk
constexpr int kFoldChunk = kFoldLoads * kBlock;   // columns staged in LDS

// Turn table layout: tab[0] = number of turns T, tab[1 + t] = first column of
// turn t (t = 0 .. T - 1), tab[1 + T] = V.
__global__ void k_fold_turns(const uint64_t* __restrict__ words, size_t V,
                             uint32_t* __restrict__ tab) {
  const size_t k = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= V) return;
  const uint64_t phi = words[0], dphi = words[1];
  // turn of column k = high word of the 128-bit phi + k * dphi
  auto turn_of = [&](uint64_t kk) {
    const uint64_t lo = kk * dphi;
    return (uint32_t)(__umul64hi(kk, dphi) + (lo + phi < lo ? 1u : 0u));
  };
  const uint32_t t = turn_of(k);
  if (k == 0 || turn_of(k - 1) != t) tab[1 + t] = (uint32_t)k;
  if (k == V - 1) {
    tab[0] = t + 1;
    tab[2 + t] = (uint32_t)V;
  }
}

// Smallest phase word whose bin is >= b: ceil(b * 2^32 / nbin) << 32.
// b >= nbin has none (`full`).
__device__ __forceinline__ uint64_t fold_threshold(unsigned b, unsigned nbin,
                                                   bool& full) {
  full = b >= nbin;
  if (full) return 0;
  return ((((uint64_t)b << 32) + nbin - 1) / nbin) << 32;
}

// Number of the turn's n_t columns that lie below the threshold X: the
// smallest m in [0, n_t] with phi_s + m * dphi >= X, where phi_s is the phase
// of the turn's first column.  No column of the turn wraps, so the products
// below are exact for every m - 1 < n_t and m < n_t.
__device__ __forceinline__ unsigned fold_lower_bound(uint64_t phi_s,
                                                     uint64_t dphi,
                                                     double inv_dphi,
                                                     unsigned n_t, uint64_t X,
                                                     bool full) {
  if (full) return n_t;
  if (X <= phi_s) return 0;
  if (dphi == 0) return n_t;
  const double e = (double)(X - phi_s) * inv_dphi;
  unsigned m = e >= (double)n_t ? n_t : (unsigned)e;
  while (m > 0 && phi_s + (uint64_t)(m - 1) * dphi >= X) --m;
  while (m < n_t && phi_s + (uint64_t)m * dphi < X) ++m;
  return m;
}

// hits[b] += columns of bin b, weights[c] += V for an unflagged row: thread i
// owns hits[i] and weights[i].
__global__ void k_fold_counts(const uint64_t* __restrict__ words,
                              const uint32_t* __restrict__ tab,
                              const uint8_t* __restrict__ flags, size_t S,
                              size_t V, unsigned nbin,
                              uint64_t* __restrict__ hits,
                              uint64_t* __restrict__ weights) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < S && !(flags && flags[i])) weights[i] += V;
  if (i >= nbin) return;
  const uint64_t phi = words[0], dphi = words[1];
  const double inv = dphi ? 1.0 / (double)dphi : 0.0;
  bool full0, full1;
  const uint64_t X0 = fold_threshold((unsigned)i, nbin, full0);
  const uint64_t X1 = fold_threshold((unsigned)i + 1, nbin, full1);
  const uint32_t n_turns = tab[0];
  uint64_t n = 0;
  for (uint32_t t = 0; t < n_turns; ++t) {
    const uint32_t ts = tab[1 + t], n_t = tab[2 + t] - ts;
    const uint64_t phi_s = phi + (uint64_t)ts * dphi;
    n += fold_lower_bound(phi_s, dphi, inv, n_t, X1, full1) -
         fold_lower_bound(phi_s, dphi, inv, n_t, X0, full0);
  }
  if (n) hits[i] += n;
}

// tiles_b bin tiles per row (fastest over blockIdx.x, so neighbouring
// workgroups read neighbouring spans of the same row).
__global__ void __launch_bounds__(kBlock)
k_fold_accumulate(const float2* __restrict__ wf,
                  const uint8_t* __restrict__ flags, size_t L, unsigned nbin,
                  const uint64_t* __restrict__ words,
                  const uint32_t* __restrict__ tab, unsigned tiles_b,
                  double* __restrict__ acc) {
  __shared__ unsigned lbs[kBlock + 1];
  __shared__ float pw[2 * kFoldChunk];
  const size_t row = blockIdx.x / tiles_b;
  const unsigned tid = threadIdx.x;
  const unsigned b0 = (blockIdx.x % tiles_b) * kBlock;
  const unsigned b = b0 + tid;
  if (flags && flags[row]) return;  // the whole workgroup: a flagged row adds 0

  const uint64_t phi = words[0], dphi = words[1];
  const double inv = dphi ? 1.0 / (double)dphi : 0.0;
  bool full, full_end = false;
  const uint64_t X = fold_threshold(b, nbin, full);
  // thread 0 also bounds the tile from above
  const uint64_t X_end =
      tid == 0 ? fold_threshold(b0 + kBlock, nbin, full_end) : 0;
  const float2* __restrict__ rowp = wf + row * L;
  const uint32_t n_turns = tab[0];

  double total = 0.0;
  bool any = false;
  unsigned half = 0;
  for (uint32_t t = 0; t < n_turns; ++t) {
    const uint32_t ts = tab[1 + t], n_t = tab[2 + t] - ts;
    const uint64_t phi_s = phi + (uint64_t)ts * dphi;
    lbs[tid] = fold_lower_bound(phi_s, dphi, inv, n_t, X, full);
    if (tid == 0)
      lbs[kBlock] = fold_lower_bound(phi_s, dphi, inv, n_t, X_end, full_end);
    __syncthreads();
    const uint32_t lo = ts + lbs[tid], hi = ts + lbs[tid + 1];
    const uint32_t span_lo = ts + lbs[0], span_hi = ts + lbs[kBlock];
    __syncthreads();  // lbs is rewritten next turn

    // Chunks alternate between the two halves of pw: the loads of the next
    // chunk are in flight while this one is summed, and one barrier per chunk
    // is enough (a half is rewritten two chunks later, past the barrier that
    // every reader of it has to reach first).
    float run = 0.0f;
    float2 v[kFoldLoads];
    auto load = [&](uint32_t c0) {
      // span_hi <= V <= L: every load stays in the row
#pragma unroll
      for (int i = 0; i < kFoldLoads; ++i) {
        const uint32_t k = c0 + tid + i * kBlock;
        v[i] = k < span_hi ? rowp[k] : make_float2(0.0f, 0.0f);
      }
    };
    if (span_lo < span_hi) load(span_lo);
    for (uint32_t c0 = span_lo; c0 < span_hi; c0 += kFoldChunk) {
      float* buf = pw + half * kFoldChunk;
      half ^= 1u;
#pragma unroll
      for (int i = 0; i < kFoldLoads; ++i) buf[tid + i * kBlock] = norm2(v[i]);
      __syncthreads();
      const uint32_t c1 = c0 + kFoldChunk;
      if (c1 < span_hi) load(c1);
      const uint32_t k0 = lo > c0 ? lo : c0;
      const uint32_t k1 = hi < c1 ? hi : c1;
      for (uint32_t k = k0; k < k1; ++k) run += buf[k - c0];
    }
    if (hi > lo) {
      total += (double)run;
      any = true;
    }
  }
  if (any) acc[row * nbin + b] += total;  // any implies b < nbin
}

}  // namespace

size_t fold_table_words(size_t V) { return V + 2; }

hipError_t fold_block(const float2* wf, const uint8_t* flags, size_t S,
                      size_t L, size_t V, size_t nbin, const uint64_t* words,
                      uint32_t* table, double* acc, uint64_t* hits,
                      uint64_t* weights, hipStream_t stream) {
  if (S == 0 || V == 0 || V > L || V >= (1ull << 31) || nbin < kFoldMinBins ||
      nbin > kFoldMaxBins)
    return hipErrorInvalidValue;
  const size_t tiles_b = (nbin + kBlock - 1) / kBlock;
  if (S * tiles_b >= (1ull << 31)) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_fold_turns, dim3((uint32_t)((V + kBlock - 1) / kBlock)),
                     dim3(kBlock), 0, stream, words, V, table);
  const size_t n_cnt = S > nbin ? S : nbin;
  hipLaunchKernelGGL(k_fold_counts,
                     dim3((uint32_t)((n_cnt + kBlock - 1) / kBlock)),
                     dim3(kBlock), 0, stream, words, table, flags, S, V,
                     (unsigned)nbin, hits, weights);
  hipLaunchKernelGGL(k_fold_accumulate, dim3((uint32_t)(S * tiles_b)),
                     dim3(kBlock), 0, stream, wf, flags, L, (unsigned)nbin,
                     words, table, (unsigned)tiles_b, acc);
  SRTB_CHECK_LAUNCH();
  return hipSuccess;
}

}  // namespace srtb_hip
