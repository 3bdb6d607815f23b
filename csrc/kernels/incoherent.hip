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

}  // namespace srtb_hip
