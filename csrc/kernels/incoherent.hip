// Incoherent DM-offset search on the filterbank power plane (no reference
// counterpart; definition in docs/ARCHITECTURE.md, "Incoherent DM-offset
// search").
//
// incoh_dedisperse: Y[t][j] = sum_c W[j + d[t][c]][c].  One wave owns
// kIncohRowsPerWave consecutive output rows of one trial and one channel
// chunk; its lanes run over the chunk's channels (4 adjacent channels per
// lane and step where C is a multiple of 4, else 1), so a lane reads its
// delays once and then its elements of every row, and the 64 lanes of a load
// touch one contiguous run wherever the delays of adjacent channels agree (a
// physical table is piecewise constant in c).  A lane adds its channels in
// ascending order, a fixed shuffle tree combines the lanes, and a second
// kernel adds the chunks in chunk order: the order of summation depends on C,
// the buffers' 16-byte alignment and the constants below only, never on the
// table or the data.  No atomics.
//
// incoh_detect: one workgroup per trial.  The fp64 inclusive scan of the
// mean-subtracted row lives in LDS (R doubles, up to kIncohMaxRows = 128 KiB
// of the 160 KiB of a gfx950 CU, which leaves such a workgroup the CU to
// itself); every boxcar length then takes two passes over it, sum of squares
// + ordered maximum, and the count above the threshold.
//
// incoh_norm_update / incoh_norm_apply: the optional per-channel
// normalisation of the rows on their way into the history ring.  update reads
// the block's [R][C] plane once for the fp64 block statistics (row chunks in
// fixed order) and advances the running mean, variance and gain; apply writes
// (x - mean) * gain into the ring in place of the device-to-device copy.

#include "../include/srtb_kernels.h"
#include "common.h"

#include <cmath>

namespace srtb_hip {

namespace {

constexpr int kIncohRowsPerWave = 8;
constexpr int kIncohWaves = kBlock / 64;
constexpr int kIncohRowsPerBlock = kIncohRowsPerWave * kIncohWaves;

constexpr int kDetectBlock = 1024;
constexpr int kDetectWaves = kDetectBlock / 64;

// grid: x = trial, y = row tile, z = channel chunk.  out is Y itself when the
// grid has one chunk, else the partials [chunk][T][R].  The trial is the
// fastest grid index, so the workgroups in flight at any time are all the
// trials of a few row tiles: they read the same few hundred rows, which stay
// in L2, instead of every trial streaming the whole plane through it.
//
// VEC4 (C a multiple of 4): a lane owns 4 adjacent channels per step.  Where
// their delays agree, which is nearly everywhere in a physical table, the four
// elements of a row are one 16-byte load; otherwise four scalar loads.  Both
// ways add the same four values in the same order, so the path a lane takes
// does not show in the result.
template <bool VEC4>
__global__ void __launch_bounds__(kBlock)
k_incoh_dedisperse(const float* __restrict__ win, size_t ring_rows,
                   size_t row0, const int* __restrict__ delays, size_t T,
                   size_t R, size_t C, float* __restrict__ out) {
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const size_t t = blockIdx.x;
  const size_t j0 = (size_t)blockIdx.y * kIncohRowsPerBlock +
                    (size_t)wave * kIncohRowsPerWave;
  if (j0 >= R) return;  // whole wave: no barrier below
  const size_t c_lo = (size_t)blockIdx.z * kIncohChannelChunk;
  const size_t c_hi = c_lo + kIncohChannelChunk < C ? c_lo + kIncohChannelChunk
                                                    : C;
  const int* __restrict__ d_row = delays + t * C;

  float acc[kIncohRowsPerWave];
#pragma unroll
  for (int r = 0; r < kIncohRowsPerWave; ++r) acc[r] = 0.f;

  // rows past R repeat row R - 1 (in bounds) and are not stored
  size_t jr[kIncohRowsPerWave];
#pragma unroll
  for (int r = 0; r < kIncohRowsPerWave; ++r)
    jr[r] = row0 + (j0 + r < R ? j0 + r : R - 1);

  // ring row of window row jr + d; jr + d < 2 * ring_rows
  auto ring = [ring_rows](size_t w) { return w >= ring_rows ? w - ring_rows : w; };

  if (VEC4) {
    // c_lo, c_hi and C are multiples of 4: whole groups, 16-byte aligned
    for (size_t c = c_lo + 4 * (size_t)lane; c < c_hi; c += 4 * 64) {
      const int4 d = *reinterpret_cast<const int4*>(d_row + c);
      if (d.x == d.y && d.y == d.z && d.z == d.w) {
#pragma unroll
        for (int r = 0; r < kIncohRowsPerWave; ++r) {
          const float4 x = *reinterpret_cast<const float4*>(
              win + ring(jr[r] + (size_t)d.x) * C + c);
          acc[r] += x.x;
          acc[r] += x.y;
          acc[r] += x.z;
          acc[r] += x.w;
        }
      } else {
#pragma unroll
        for (int r = 0; r < kIncohRowsPerWave; ++r) {
          acc[r] += win[ring(jr[r] + (size_t)d.x) * C + c];
          acc[r] += win[ring(jr[r] + (size_t)d.y) * C + c + 1];
          acc[r] += win[ring(jr[r] + (size_t)d.z) * C + c + 2];
          acc[r] += win[ring(jr[r] + (size_t)d.w) * C + c + 3];
        }
      }
    }
  } else {
    for (size_t c = c_lo + lane; c < c_hi; c += 64) {
      const size_t d = (size_t)d_row[c];
#pragma unroll
      for (int r = 0; r < kIncohRowsPerWave; ++r)
        acc[r] += win[ring(jr[r] + d) * C + c];
    }
  }

  float* __restrict__ o = out + ((size_t)blockIdx.z * T + t) * R;
#pragma unroll
  for (int r = 0; r < kIncohRowsPerWave; ++r) {
    const float s = wave_reduce_sum(acc[r]);
    if (lane == 0 && j0 + r < R) o[j0 + r] = s;
  }
}

__global__ void k_incoh_combine(const float* __restrict__ partial,
                                size_t cells, int chunks,
                                float* __restrict__ y) {
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < cells;
       i += stride) {
    float s = partial[i];
    for (int k = 1; k < chunks; ++k) s += partial[(size_t)k * cells + i];
    y[i] = s;
  }
}

// ---- detection ----

struct PeakD {
  double v;
  unsigned i;
};

__device__ __forceinline__ PeakD peak_better(PeakD a, PeakD b) {
  return (b.v > a.v || (b.v == a.v && b.i < a.i)) ? b : a;
}

__device__ __forceinline__ PeakD wave_reduce_peak(PeakD p) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    PeakD q;
    q.v = __shfl_down(p.v, off, 64);
    q.i = __shfl_down(p.i, off, 64);
    p = peak_better(p, q);
  }
  return p;
}

struct DetectShared {
  double sum[kDetectWaves];
  double peak_v[kDetectWaves];
  unsigned peak_i[kDetectWaves];
  unsigned count[kDetectWaves];
};

// sum over the workgroup in a fixed order, returned to every thread
__device__ inline double detect_block_sum(double v, DetectShared& sh) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  v = wave_reduce_sum(v);
  __syncthreads();
  if (lane == 0) sh.sum[wave] = v;
  __syncthreads();
  double s = 0.0;
  for (int w = 0; w < kDetectWaves; ++w) s += sh.sum[w];
  return s;
}

__global__ void __launch_bounds__(kDetectBlock)
k_incoh_detect(const float* __restrict__ Y, size_t R, int n_lengths,
               double snr, double* __restrict__ out_peak,
               unsigned* __restrict__ out_index, double* __restrict__ out_rms,
               unsigned* __restrict__ out_count, double* __restrict__ out_mu) {
  extern __shared__ double cs[];  // [R]
  __shared__ DetectShared sh;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const size_t t = blockIdx.x;
  const float* __restrict__ y = Y + t * R;

  // mean
  double s = 0.0;
  for (size_t j = tid; j < R; j += kDetectBlock) s += (double)y[j];
  const double mu = detect_block_sum(s, sh) / (double)R;

  // inclusive scan of z = y - mu: a thread scans one contiguous segment, the
  // segment totals are scanned across the workgroup
  const size_t seg = (R + kDetectBlock - 1) / kDetectBlock;
  const size_t lo = (size_t)tid * seg < R ? (size_t)tid * seg : R;
  const size_t hi = lo + seg < R ? lo + seg : R;
  double run = 0.0;
  for (size_t j = lo; j < hi; ++j) {
    run += (double)y[j] - mu;
    cs[j] = run;
  }
  double incl = run;  // inclusive scan over the wave's lanes
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const double up = __shfl_up(incl, off, 64);
    if (lane >= off) incl += up;
  }
  __syncthreads();
  if (lane == 63) sh.sum[wave] = incl;
  __syncthreads();
  double offset = incl - run;  // exclusive within the wave
  for (int w = 0; w < wave; ++w) offset += sh.sum[w];
  for (size_t j = lo; j < hi; ++j) cs[j] += offset;
  __syncthreads();

  for (int l = 0; l < n_lengths; ++l) {
    const size_t len = (size_t)1 << l;
    const size_t n = l == 0 ? R : (len < R ? R - len : 0);
    PeakD pk;
    pk.v = -INFINITY;
    pk.i = 0xFFFFFFFFu;
    double ss = 0.0;
    for (size_t i = tid; i < n; i += kDetectBlock) {
      const double b = l == 0 ? (double)y[i] - mu : cs[i + len] - cs[i];
      ss += b * b;
      if (b > pk.v) {
        pk.v = b;
        pk.i = (unsigned)i;
      }
    }
    const double sumsq = detect_block_sum(ss, sh);
    pk = wave_reduce_peak(pk);
    if (lane == 0) {
      sh.peak_v[wave] = pk.v;
      sh.peak_i[wave] = pk.i;
    }
    const double rms = n ? sqrt(sumsq / (double)n) : 0.0;
    const double thr = snr * rms;
    unsigned cnt = 0;
    for (size_t i = tid; i < n; i += kDetectBlock) {
      const double b = l == 0 ? (double)y[i] - mu : cs[i + len] - cs[i];
      cnt += b > thr ? 1u : 0u;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) cnt += __shfl_down(cnt, off, 64);
    if (lane == 0) sh.count[wave] = cnt;
    __syncthreads();
    if (tid == 0) {
      PeakD best;
      best.v = sh.peak_v[0];
      best.i = sh.peak_i[0];
      unsigned total = sh.count[0];
      for (int w = 1; w < kDetectWaves; ++w) {
        PeakD q;
        q.v = sh.peak_v[w];
        q.i = sh.peak_i[w];
        best = peak_better(best, q);
        total += sh.count[w];
      }
      const size_t o = t * (size_t)n_lengths + l;
      out_peak[o] = best.v;
      out_index[o] = best.i;
      out_rms[o] = rms;
      out_count[o] = total;
    }
    // the next length's first barrier (in detect_block_sum) comes before any
    // write to sh.peak_* / sh.count, so thread 0's reads above are safe
  }
  if (tid == 0) out_mu[t] = mu;
}

// ---- per-channel normalisation ----

constexpr int kIncohNormChunks = 64;      // row chunks of the block statistics
constexpr int kIncohNormRowsPerThread = 8;  // rows a thread of apply walks

// a * b rounded on its own.  The build contracts a * b + c across statements
// and ignores the contract pragma; an fma with a zero addend is one rounding
// of the product and is not merged into the addition that follows.
__device__ __forceinline__ double mul_rn(double a, double b) {
  return __builtin_fma(a, b, 0.0);
}

// grid: x = 256 channels, y = row chunk.  Lanes run along c, so a wave's load
// of a row is one contiguous run.  partials: [chunks][2][C]; a chunk past the
// last row writes zeros.
__global__ void __launch_bounds__(kBlock)
k_incoh_norm_partial(const float* __restrict__ P, size_t R, size_t C,
                     int n_chunks, double* __restrict__ partials) {
  const size_t c = (size_t)blockIdx.x * kBlock + threadIdx.x;
  if (c >= C) return;
  const int chunk = blockIdx.y;
  const size_t rows_per = (R + n_chunks - 1) / n_chunks;
  const size_t r0 = min((size_t)chunk * rows_per, R);
  const size_t r1 = min(r0 + rows_per, R);
  const double x0 = (double)P[c];
  double s = 0.0, s2 = 0.0;
#pragma unroll 8
  for (size_t r = r0; r < r1; ++r) {
    const double d = (double)P[r * C + c] - x0;
    s += d;
    s2 += mul_rn(d, d);
  }
  partials[((size_t)chunk * 2 + 0) * C + c] = s;
  partials[((size_t)chunk * 2 + 1) * C + c] = s2;
}

// one thread per channel: the chunks in chunk order, then the running state
__global__ void __launch_bounds__(kBlock)
k_incoh_norm_state(const float* __restrict__ P, size_t R, size_t C,
                   int n_chunks, const double* __restrict__ partials,
                   double alpha, double* __restrict__ M,
                   double* __restrict__ V, float* __restrict__ G) {
  const size_t c = (size_t)blockIdx.x * kBlock + threadIdx.x;
  if (c >= C) return;
  double s = 0.0, s2 = 0.0;
  for (int k = 0; k < n_chunks; ++k) {
    s += partials[((size_t)k * 2 + 0) * C + c];
    s2 += partials[((size_t)k * 2 + 1) * C + c];
  }
  const double ds = s / (double)R;  // mean of x - x0
  const double m = (double)P[c] + ds;
  double v = s2 / (double)R - mul_rn(ds, ds);
  v = v > 0.0 ? v : 0.0;
  const double m_run = M[c], v_run = V[c];
  const double m_new = m_run + mul_rn(alpha, m - m_run);
  const double v_new = v_run + mul_rn(alpha, v - v_run);
  M[c] = m_new;
  V[c] = v_new;
  G[c] = v_new > 0.0 ? (float)(1.0 / sqrt(v_new)) : 0.0f;
}

// one workgroup: #{G > 0}, a fixed shuffle tree per wave, the waves in order
__global__ void __launch_bounds__(kBlock)
k_incoh_norm_live(const float* __restrict__ G, size_t C,
                  unsigned* __restrict__ live) {
  __shared__ unsigned per_wave[kBlock / 64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  unsigned n = 0;
  for (size_t c = threadIdx.x; c < C; c += kBlock) n += G[c] > 0.0f ? 1u : 0u;
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) n += __shfl_down(n, off, 64);
  if (lane == 0) per_wave[wave] = n;
  __syncthreads();
  if (threadIdx.x == 0) {
    unsigned total = 0;
    for (int w = 0; w < kBlock / 64; ++w) total += per_wave[w];
    *live = total;
  }
}

__device__ __forceinline__ float norm1(float x, float m, float g) {
  // a subtraction, then a multiplication: nothing here can contract
  return (x - m) * g;
}

// grid: x = 256 lanes of channels (4 adjacent ones per lane with VEC4), y =
// kIncohNormRowsPerThread rows.  A thread keeps (float)M and G of its channels
// in registers over its rows.  Block row r goes to ring row
// (write_row + r) mod ring_rows.
template <bool VEC4>
__global__ void __launch_bounds__(kBlock)
k_incoh_norm_apply(const float* __restrict__ P, size_t R, size_t C,
                   const double* __restrict__ M, const float* __restrict__ G,
                   float* __restrict__ ring, size_t ring_rows,
                   size_t write_row) {
  const size_t c = ((size_t)blockIdx.x * kBlock + threadIdx.x) * (VEC4 ? 4 : 1);
  if (c >= C) return;
  const size_t r0 = (size_t)blockIdx.y * kIncohNormRowsPerThread;
  const size_t r1 = min(r0 + kIncohNormRowsPerThread, R);
  if (VEC4) {
    // C is a multiple of 4: c + 3 < C
    const float4 g = *reinterpret_cast<const float4*>(G + c);
    const float m0 = (float)M[c], m1 = (float)M[c + 1], m2 = (float)M[c + 2],
                m3 = (float)M[c + 3];
    for (size_t r = r0; r < r1; ++r) {
      const float4 x = *reinterpret_cast<const float4*>(P + r * C + c);
      size_t w = write_row + r;
      if (w >= ring_rows) w -= ring_rows;
      float4 y;
      y.x = norm1(x.x, m0, g.x);
      y.y = norm1(x.y, m1, g.y);
      y.z = norm1(x.z, m2, g.z);
      y.w = norm1(x.w, m3, g.w);
      *reinterpret_cast<float4*>(ring + w * C + c) = y;
    }
  } else {
    const float g = G[c], m = (float)M[c];
    for (size_t r = r0; r < r1; ++r) {
      size_t w = write_row + r;
      if (w >= ring_rows) w -= ring_rows;
      ring[w * C + c] = norm1(P[r * C + c], m, g);
    }
  }
}

}  // namespace

int incoh_chunks(size_t C) {
  return (int)((C + kIncohChannelChunk - 1) / kIncohChannelChunk);
}

size_t incoh_partials(size_t T, size_t R, size_t C) {
  const int k = incoh_chunks(C);
  return k > 1 ? (size_t)k * T * R : 0;
}

int incoh_lengths(size_t max_boxcar) {
  int n = 0;
  for (size_t l = 1; l <= max_boxcar && n < kIncohMaxLengths; l *= 2) ++n;
  return n;
}

hipError_t incoh_dedisperse(const float* window, size_t ring_rows, size_t row0,
                            const int* delays, size_t T, size_t R, size_t C,
                            float* partials, float* Y, hipStream_t stream) {
  if (T < 1 || T > kIncohMaxTrials || R < 1 || C < 1 || ring_rows < R ||
      row0 >= ring_rows || ring_rows - R > kIncohMaxDelay ||
      ring_rows * C * sizeof(float) > kIncohMaxWindowBytes)
    return hipErrorInvalidValue;
  const int chunks = incoh_chunks(C);
  if (chunks > 65535 || (chunks > 1 && !partials)) return hipErrorInvalidValue;
  const size_t tiles = (R + kIncohRowsPerBlock - 1) / kIncohRowsPerBlock;
  if (tiles > 65535) return hipErrorInvalidValue;
  const dim3 grid((uint32_t)T, (uint32_t)tiles, (uint32_t)chunks);
  float* out = chunks > 1 ? partials : Y;
  // 16-byte loads need rows and table rows that start on 16 bytes
  const bool vec4 = C % 4 == 0 &&
                    reinterpret_cast<uintptr_t>(window) % 16 == 0 &&
                    reinterpret_cast<uintptr_t>(delays) % 16 == 0;
  if (vec4)
    hipLaunchKernelGGL(k_incoh_dedisperse<true>, grid, dim3(kBlock), 0, stream,
                       window, ring_rows, row0, delays, T, R, C, out);
  else
    hipLaunchKernelGGL(k_incoh_dedisperse<false>, grid, dim3(kBlock), 0,
                       stream, window, ring_rows, row0, delays, T, R, C, out);
  if (chunks > 1)
    hipLaunchKernelGGL(k_incoh_combine, grid_for(T * R), dim3(kBlock), 0,
                       stream, partials, T * R, chunks, Y);
  SRTB_CHECK_LAUNCH();
  return hipSuccess;
}

hipError_t incoh_detect(const float* Y, size_t T, size_t R, int n_lengths,
                        double snr, double* out_peak, unsigned* out_index,
                        double* out_rms, unsigned* out_count, double* out_mu,
                        hipStream_t stream) {
  if (T < 1 || T > kIncohMaxTrials || R < kIncohMinRows || R > kIncohMaxRows ||
      n_lengths < 1 || n_lengths > kIncohMaxLengths)
    return hipErrorInvalidValue;
  const size_t lds = R * sizeof(double);
  // above 64 KiB of dynamic LDS the runtime wants the size declared; the
  // attribute is per device, so it is set on every call (a host-side store)
  const hipError_t attr = hipFuncSetAttribute(
      reinterpret_cast<const void*>(k_incoh_detect),
      hipFuncAttributeMaxDynamicSharedMemorySize,
      (int)(kIncohMaxRows * sizeof(double)));
  if (attr != hipSuccess) return attr;
  hipLaunchKernelGGL(k_incoh_detect, dim3((uint32_t)T), dim3(kDetectBlock),
                     lds, stream, Y, R, n_lengths, snr, out_peak, out_index,
                     out_rms, out_count, out_mu);
  SRTB_CHECK_LAUNCH();
  return hipSuccess;
}

size_t incoh_norm_partials(size_t C) {
  return (size_t)kIncohNormChunks * 2 * C;
}

hipError_t incoh_norm_update(const float* plane, size_t R, size_t C,
                             double alpha, double* partials, double* M,
                             double* V, float* G, unsigned* live,
                             hipStream_t stream) {
  if (R == 0 || C == 0 || !plane || !partials || !M || !V || !G || !live)
    return hipErrorInvalidValue;
  const size_t gx = (C + kBlock - 1) / kBlock;
  if (gx >= (1ull << 31)) return hipErrorInvalidValue;
  const int chunks = (int)(R < (size_t)kIncohNormChunks ? R : kIncohNormChunks);
  hipLaunchKernelGGL(k_incoh_norm_partial,
                     dim3((uint32_t)gx, (uint32_t)chunks), dim3(kBlock), 0,
                     stream, plane, R, C, chunks, partials);
  hipLaunchKernelGGL(k_incoh_norm_state, dim3((uint32_t)gx), dim3(kBlock), 0,
                     stream, plane, R, C, chunks, partials, alpha, M, V, G);
  hipLaunchKernelGGL(k_incoh_norm_live, dim3(1), dim3(kBlock), 0, stream, G,
                     C, live);
  SRTB_CHECK_LAUNCH();
  return hipSuccess;
}

hipError_t incoh_norm_apply(const float* plane, size_t R, size_t C,
                            const double* M, const float* G, float* ring,
                            size_t ring_rows, size_t write_row,
                            hipStream_t stream) {
  if (R == 0 || C == 0 || ring_rows < R || write_row >= ring_rows || !plane ||
      !M || !G || !ring)
    return hipErrorInvalidValue;
  const size_t tiles =
      (R + kIncohNormRowsPerThread - 1) / kIncohNormRowsPerThread;
  if (tiles > 65535) return hipErrorInvalidValue;
  auto aligned16 = [](const void* p) {
    return reinterpret_cast<uintptr_t>(p) % 16 == 0;
  };
  // 16-byte accesses need rows (of the block and of the ring) and a gain
  // vector that start on 16 bytes
  const bool vec4 =
      C % 4 == 0 && aligned16(plane) && aligned16(ring) && aligned16(G);
  const size_t lanes = vec4 ? C / 4 : C;
  const size_t gx = (lanes + kBlock - 1) / kBlock;
  if (gx >= (1ull << 31)) return hipErrorInvalidValue;
  const dim3 grid((uint32_t)gx, (uint32_t)tiles);
  if (vec4)
    hipLaunchKernelGGL(k_incoh_norm_apply<true>, grid, dim3(kBlock), 0, stream,
                       plane, R, C, M, G, ring, ring_rows, write_row);
  else
    hipLaunchKernelGGL(k_incoh_norm_apply<false>, grid, dim3(kBlock), 0,
                       stream, plane, R, C, M, G, ring, ring_rows, write_row);
  SRTB_CHECK_LAUNCH();
  return hipSuccess;
}

}  // namespace srtb_hip
