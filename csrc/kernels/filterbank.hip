// Filterbank output kernels: the block's coherently dedispersed [S][L]
// waterfall -> a time-major, channelised, time-integrated power plane
// P[R][C] (SIGPROC order: channel fastest, descending frequency), its
// per-channel statistics and the 8-bit quantisation.  Definition:
// docs/ARCHITECTURE.md, "Filterbank output".  NumPy oracle:
// srtb_amd.ref.filterbank_block / filterbank_quantize.
//
// MI355X design notes:
//  - filterbank_detect is a transposing reduce.  Loads run along time (the
//    waterfall's fast axis): the G = min(tscrunch/2, 64) lanes that share one
//    output cell read consecutive float4 (two complex samples each), so a
//    wave's load instruction covers one contiguous 1 KB run of a waterfall
//    row.  Each lane sums its share of the tscrunch x fscrunch cell in a
//    register, an xor-shuffle tree folds the G lanes, and the cell goes into
//    a [rows][33] LDS tile whose read-out runs along the channel axis, so the
//    global stores are contiguous in c.  No atomics; the summation order
//    depends only on the shape.
//  - tscrunch = 1 has no lanes to fold: one float4 is two output rows.
//  - the statistics are the project's two-stage scheme: fp64 partials per
//    fixed row chunk, combined in chunk order.

#include "common.h"
#include "../include/srtb_kernels.h"

namespace srtb_hip {

namespace {

constexpr int kFilTileC = 32;      // output channels per tile
constexpr int kFilTileR = 32;      // output cells along time per tile
constexpr int kFilTileRows = 64;   // LDS rows (tscrunch = 1: two per cell)
constexpr int kFilStatChunks = 64;  // row chunks of the statistics
constexpr int kFilStatBlock = 64;

__device__ __forceinline__ float power4(float4 v) {
  return (v.x * v.x + v.y * v.y) + (v.z * v.z + v.w * v.w);
}

// tiles_r tiles along time (fastest over blockIdx.x), tiles_c along channel.
// q4 = tscrunch / 2 float4 per output cell and row (0 for tscrunch = 1),
// G = min(q4, 64) lanes per cell.
__global__ void __launch_bounds__(kBlock)
k_filterbank_detect(const float2* __restrict__ wf,
                    const uint8_t* __restrict__ flags, size_t S, size_t L,
                    size_t V, unsigned q4, unsigned G, unsigned fscrunch,
                    int reverse, size_t R, size_t C, unsigned tiles_r,
                    float* __restrict__ out) {
  __shared__ float tile[kFilTileRows][kFilTileC + 1];
  const unsigned tile_r = blockIdx.x % tiles_r;
  const unsigned tile_c = blockIdx.x / tiles_r;
  const size_t c0 = (size_t)tile_c * kFilTileC;
  const unsigned tid = threadIdx.x;

  if (q4 == 0) {
    // tscrunch = 1: cell = one float4 column of one channel, two output rows
    const size_t r0 = (size_t)tile_r * kFilTileRows;
#pragma unroll
    for (unsigned it = 0; it < kFilTileC * kFilTileR / kBlock; ++it) {
      const unsigned o = tid + it * kBlock;
      const unsigned j = o % kFilTileR, cl = o / kFilTileR;
      const size_t c = c0 + cl, r = r0 + 2 * (size_t)j;
      float a0 = 0.0f, a1 = 0.0f;
      if (c < C && r < R) {
        const size_t row0 = reverse ? S - (c + 1) * fscrunch : c * fscrunch;
        for (unsigned f = 0; f < fscrunch; ++f) {
          const size_t row = row0 + f;
          if (flags && flags[row]) continue;
          // r is even and r < V <= L with L even: the float4 stays in the row
          const float4 v =
              *reinterpret_cast<const float4*>(wf + row * L + r);
          a0 += v.x * v.x + v.y * v.y;
          a1 += v.z * v.z + v.w * v.w;
        }
      }
      tile[2 * j][cl] = a0;
      tile[2 * j + 1][cl] = a1;
    }
  } else {
    const size_t r0 = (size_t)tile_r * kFilTileR;
    const unsigned g = tid % G;           // lane within the cell's group
    const unsigned per_it = kBlock / G;   // cells per iteration
    const unsigned n_it = kFilTileC * kFilTileR / per_it;
    const unsigned n_i = q4 / G;          // float4 per lane, row and cell
#pragma unroll 4
    for (unsigned it = 0; it < n_it; ++it) {
      const unsigned o = tid / G + it * per_it;
      const unsigned rl = o % kFilTileR, cl = o / kFilTileR;
      const size_t c = c0 + cl, r = r0 + rl;
      float acc = 0.0f;
      if (c < C && r < R) {
        const size_t row0 = reverse ? S - (c + 1) * fscrunch : c * fscrunch;
        // (r + 1) * tscrunch <= V <= L: every float4 stays in the row
        const size_t t4 = r * q4 + g;
        for (unsigned f = 0; f < fscrunch; ++f) {
          const size_t row = row0 + f;
          if (flags && flags[row]) continue;
          const float4* p =
              reinterpret_cast<const float4*>(wf + row * L) + t4;
          for (unsigned i = 0; i < n_i; ++i) acc += power4(p[(size_t)i * G]);
        }
      }
      // fold the cell's G lanes (G is a power of two <= 64 dividing the wave,
      // all lanes take part: the trip counts above are uniform)
      for (unsigned off = G >> 1; off > 0; off >>= 1)
        acc += __shfl_xor(acc, (int)off, 64);
      if (g == 0) tile[rl][cl] = acc;
    }
  }
  __syncthreads();

  // read-out along the channel axis
  const unsigned rows_here = q4 == 0 ? kFilTileRows : kFilTileR;
  const size_t rbase = (size_t)tile_r * rows_here;
  const unsigned cl = tid % kFilTileC;
  const size_t c = c0 + cl;
  if (c < C) {
    for (unsigned rl = tid / kFilTileC; rl < rows_here;
         rl += kBlock / kFilTileC) {
      const size_t r = rbase + rl;
      if (r < R) out[r * C + c] = tile[rl][cl];
    }
  }
}

// ---- polarization products (docs/ARCHITECTURE.md, "Polarization products")
// Two waterfalls A = x+iy, B = u+iv of the same sky -> AA, BB, CR, CI per cell.
// NA = 1 keeps only AA+BB (state I), NA = 4 keeps all four; v holds two
// complex samples of each waterfall.
template <int NA>
__device__ __forceinline__ void pol_acc2(float (&acc)[NA], float4 a,
                                         float4 b) {
  if constexpr (NA == 1) {
    acc[0] += power4(a) + power4(b);
  } else {
    acc[0] += power4(a);
    acc[1] += power4(b);
    acc[2] += (a.x * b.x + a.y * b.y) + (a.z * b.z + a.w * b.w);
    acc[3] += (a.y * b.x - a.x * b.y) + (a.w * b.z - a.z * b.w);
  }
}

// one complex sample of each (the tscrunch = 1 path)
template <int NA>
__device__ __forceinline__ void pol_acc1(float (&acc)[NA], float x, float y,
                                         float u, float v) {
  if constexpr (NA == 1) {
    acc[0] += (x * x + y * y) + (u * u + v * v);
  } else {
    acc[0] += x * x + y * y;
    acc[1] += u * u + v * v;
    acc[2] += x * u + y * v;
    acc[3] += y * u - x * v;
  }
}

// k_filterbank_detect's tiling with NA accumulators per cell and an
// [NA][rows][33] LDS tile; out is [R][NA][C].  iquv (NA = 4 only): the four
// cell sums leave as I, Q, U, V, one fp32 operation each.  The tile is dynamic
// LDS sized by the launcher: 64 rows are needed only by the tscrunch = 1 path,
// and with 32 the four-product tile is 16.5 KB instead of 33 KB, which is what
// lets eight workgroups instead of four share a CU.
template <int NA>
__global__ void __launch_bounds__(kBlock)
k_filterbank_detect_pol(const float2* __restrict__ wa,
                        const float2* __restrict__ wb,
                        const uint8_t* __restrict__ fa,
                        const uint8_t* __restrict__ fb, size_t S, size_t L,
                        size_t V, unsigned q4, unsigned G, unsigned fscrunch,
                        int reverse, int iquv, size_t R, size_t C,
                        unsigned tiles_r, float* __restrict__ out) {
  extern __shared__ float pol_tile[];
  const unsigned rows_here = q4 == 0 ? kFilTileRows : kFilTileR;
  // tile[p][rl][cl]
  auto tile = [&](unsigned p, unsigned rl, unsigned cl) -> float& {
    return pol_tile[(p * rows_here + rl) * (kFilTileC + 1) + cl];
  };
  const unsigned tile_r = blockIdx.x % tiles_r;
  const unsigned tile_c = blockIdx.x / tiles_r;
  const size_t c0 = (size_t)tile_c * kFilTileC;
  const unsigned tid = threadIdx.x;

  if (q4 == 0) {
    // tscrunch = 1: cell = one float4 column of one channel, two output rows
    const size_t r0 = (size_t)tile_r * kFilTileRows;
#pragma unroll
    for (unsigned it = 0; it < kFilTileC * kFilTileR / kBlock; ++it) {
      const unsigned o = tid + it * kBlock;
      const unsigned j = o % kFilTileR, cl = o / kFilTileR;
      const size_t c = c0 + cl, r = r0 + 2 * (size_t)j;
      float a0[NA] = {}, a1[NA] = {};
      if (c < C && r < R) {
        const size_t row0 = reverse ? S - (c + 1) * fscrunch : c * fscrunch;
        for (unsigned f = 0; f < fscrunch; ++f) {
          const size_t row = row0 + f;
          if ((fa && fa[row]) || (fb && fb[row])) continue;
          // r is even and r < V <= L with L even: the float4 stays in the row
          const float4 a = *reinterpret_cast<const float4*>(wa + row * L + r);
          const float4 b = *reinterpret_cast<const float4*>(wb + row * L + r);
          pol_acc1<NA>(a0, a.x, a.y, b.x, b.y);
          pol_acc1<NA>(a1, a.z, a.w, b.z, b.w);
        }
      }
#pragma unroll
      for (int p = 0; p < NA; ++p) {
        tile(p, 2 * j, cl) = a0[p];
        tile(p, 2 * j + 1, cl) = a1[p];
      }
    }
  } else {
    const size_t r0 = (size_t)tile_r * kFilTileR;
    const unsigned g = tid % G;           // lane within the cell's group
    const unsigned per_it = kBlock / G;   // cells per iteration
    const unsigned n_it = kFilTileC * kFilTileR / per_it;
    const unsigned n_i = q4 / G;          // float4 per lane, row and cell
    for (unsigned it = 0; it < n_it; ++it) {
      const unsigned o = tid / G + it * per_it;
      const unsigned rl = o % kFilTileR, cl = o / kFilTileR;
      const size_t c = c0 + cl, r = r0 + rl;
      float acc[NA] = {};
      if (c < C && r < R) {
        const size_t row0 = reverse ? S - (c + 1) * fscrunch : c * fscrunch;
        // (r + 1) * tscrunch <= V <= L: every float4 stays in the row
        const size_t t4 = r * q4 + g;
        for (unsigned f = 0; f < fscrunch; ++f) {
          const size_t row = row0 + f;
          if ((fa && fa[row]) || (fb && fb[row])) continue;
          const float4* pa =
              reinterpret_cast<const float4*>(wa + row * L) + t4;
          const float4* pb =
              reinterpret_cast<const float4*>(wb + row * L) + t4;
          for (unsigned i = 0; i < n_i; ++i)
            pol_acc2<NA>(acc, pa[(size_t)i * G], pb[(size_t)i * G]);
        }
      }
      // fold the cell's G lanes (all lanes take part: uniform trip counts)
      for (unsigned off = G >> 1; off > 0; off >>= 1) {
#pragma unroll
        for (int p = 0; p < NA; ++p)
          acc[p] += __shfl_xor(acc[p], (int)off, 64);
      }
      if (g == 0) {
#pragma unroll
        for (int p = 0; p < NA; ++p) tile(p, rl, cl) = acc[p];
      }
    }
  }
  __syncthreads();

  // read-out along the channel axis, one run of C per product
  const size_t rbase = (size_t)tile_r * rows_here;
  const unsigned cl = tid % kFilTileC;
  const size_t c = c0 + cl;
  if (c < C) {
    for (unsigned rl = tid / kFilTileC; rl < rows_here;
         rl += kBlock / kFilTileC) {
      const size_t r = rbase + rl;
      if (r >= R) continue;
      float* o = out + r * NA * C + c;
      if constexpr (NA == 1) {
        o[0] = tile(0, rl, cl);
      } else {
        const float aa = tile(0, rl, cl), bb = tile(1, rl, cl);
        const float cr = tile(2, rl, cl), ci = tile(3, rl, cl);
        o[0] = iquv ? aa + bb : aa;
        o[C] = iquv ? aa - bb : bb;
        o[2 * C] = iquv ? cr + cr : cr;
        o[3 * C] = iquv ? ci + ci : ci;
      }
    }
  }
}

// Stage 1: sums of d = P[r][c] - P[0][c] and of d^2 over the rows of chunk
// blockIdx.y; one thread per channel, so loads run along c.  The shift by the
// channel's first sample keeps a constant channel at exactly zero variance.
__global__ void k_filterbank_stats_partial(const float* __restrict__ P,
                                           size_t R, size_t C, int n_chunks,
                                           double* __restrict__ partials) {
  const size_t c = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= C) return;
  const int chunk = blockIdx.y;
  const size_t rows_per = (R + n_chunks - 1) / n_chunks;
  const size_t r0 = (size_t)chunk * rows_per;
  const size_t r1 = min(r0 + rows_per, R);
  const double k = (double)P[c];
  double s = 0.0, s2 = 0.0;
  for (size_t r = r0; r < r1; ++r) {
    const double d = (double)P[r * C + c] - k;
    s += d;
    s2 += d * d;
  }
  partials[((size_t)chunk * 2 + 0) * C + c] = s;
  partials[((size_t)chunk * 2 + 1) * C + c] = s2;
}

__global__ void k_filterbank_stats_combine(const float* __restrict__ P,
                                           size_t R, size_t C, int n_chunks,
                                           const double* __restrict__ partials,
                                           float* __restrict__ mean,
                                           float* __restrict__ stddev) {
  const size_t c = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= C) return;
  double s = 0.0, s2 = 0.0;
  for (int k = 0; k < n_chunks; ++k) {
    s += partials[((size_t)k * 2 + 0) * C + c];
    s2 += partials[((size_t)k * 2 + 1) * C + c];
  }
  const double m = s / (double)R;
  const double var = s2 / (double)R - m * m;
  mean[c] = (float)((double)P[c] + m);
  stddev[c] = (float)sqrt(var > 0.0 ? var : 0.0);
}

__device__ __forceinline__ unsigned quantize1(float p, float mu, float sigma) {
  if (!(sigma > 0.0f)) return (unsigned)kFilterbankQuantLevel;
  const float inv = (float)kFilterbankQuantPerSigma / sigma;
  float q = rintf((p - mu) * inv + (float)kFilterbankQuantLevel);
  q = fminf(fmaxf(q, 0.0f), 255.0f);
  return (unsigned)q;
}

// four elements per thread: one float4 load, one packed 32-bit store
__global__ void k_filterbank_quantize(const float* __restrict__ P,
                                      const float* __restrict__ mean,
                                      const float* __restrict__ stddev,
                                      size_t n, size_t C,
                                      uint8_t* __restrict__ out) {
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  const size_t n4 = n / 4;
  const float4* P4 = reinterpret_cast<const float4*>(P);
  uint32_t* out4 = reinterpret_cast<uint32_t*>(out);
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4;
       i += stride) {
    const float4 v = P4[i];
    const float e[4] = {v.x, v.y, v.z, v.w};
    size_t c = (4 * i) % C;
    uint32_t w = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      w |= quantize1(e[k], mean[c], stddev[c]) << (8 * k);
      if (++c == C) c = 0;
    }
    out4[i] = w;
  }
  if (blockIdx.x == 0 && threadIdx.x < (n & 3)) {
    const size_t e = 4 * n4 + threadIdx.x;
    const size_t c = e % C;
    out[e] = (uint8_t)quantize1(P[e], mean[c], stddev[c]);
  }
}

bool is_pow2(size_t x) { return x && !(x & (x - 1)); }

}  // namespace

hipError_t filterbank_detect(const float2* wf, const uint8_t* flags, size_t S,
                             size_t L, size_t V, size_t tscrunch,
                             size_t fscrunch, bool reverse, float* out,
                             hipStream_t stream) {
  if (!is_pow2(tscrunch) || tscrunch > kFilterbankMaxTscrunch ||
      fscrunch == 0 || S % fscrunch != 0 || V > L || V < tscrunch ||
      L % 2 != 0)
    return hipErrorInvalidValue;
  const size_t R = V / tscrunch, C = S / fscrunch;
  const unsigned q4 = (unsigned)(tscrunch / 2);
  const unsigned G = q4 > 64 ? 64u : q4;
  const size_t rows_per_tile = q4 == 0 ? kFilTileRows : kFilTileR;
  const size_t tiles_r = (R + rows_per_tile - 1) / rows_per_tile;
  const size_t tiles_c = (C + kFilTileC - 1) / kFilTileC;
  if (tiles_r * tiles_c >= (1ull << 31)) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_filterbank_detect, dim3((uint32_t)(tiles_r * tiles_c)),
                     dim3(kBlock), 0, stream, wf, flags, S, L, V, q4, G,
                     (unsigned)fscrunch, reverse ? 1 : 0, R, C,
                     (unsigned)tiles_r, out);
  SRTB_CHECK_LAUNCH();
  return hipSuccess;
}

int pol_state_nifs(int pol_state) {
  if (pol_state == kPolStateI) return 1;
  if (pol_state == kPolStateAABBCRCI || pol_state == kPolStateIQUV) return 4;
  return 0;
}

hipError_t filterbank_detect_pol(const float2* wf_a, const float2* wf_b,
                                 const uint8_t* flags_a,
                                 const uint8_t* flags_b, size_t S, size_t L,
                                 size_t V, size_t tscrunch, size_t fscrunch,
                                 bool reverse, int pol_state, float* out,
                                 hipStream_t stream) {
  if (!is_pow2(tscrunch) || tscrunch > kFilterbankMaxTscrunch ||
      fscrunch == 0 || S % fscrunch != 0 || V > L || V < tscrunch ||
      L % 2 != 0 || pol_state_nifs(pol_state) == 0)
    return hipErrorInvalidValue;
  const size_t R = V / tscrunch, C = S / fscrunch;
  const unsigned q4 = (unsigned)(tscrunch / 2);
  const unsigned G = q4 > 64 ? 64u : q4;
  const size_t rows_per_tile = q4 == 0 ? kFilTileRows : kFilTileR;
  const size_t tiles_r = (R + rows_per_tile - 1) / rows_per_tile;
  const size_t tiles_c = (C + kFilTileC - 1) / kFilTileC;
  if (tiles_r * tiles_c >= (1ull << 31)) return hipErrorInvalidValue;
  const dim3 grid((uint32_t)(tiles_r * tiles_c));
  // [P][rows_per_tile][33] floats
  const size_t lds = (size_t)pol_state_nifs(pol_state) * rows_per_tile *
                     (kFilTileC + 1) * sizeof(float);
  if (pol_state == kPolStateI)
    hipLaunchKernelGGL(k_filterbank_detect_pol<1>, grid, dim3(kBlock), lds,
                       stream, wf_a, wf_b, flags_a, flags_b, S, L, V, q4, G,
                       (unsigned)fscrunch, reverse ? 1 : 0, 0, R, C,
                       (unsigned)tiles_r, out);
  else
    hipLaunchKernelGGL(k_filterbank_detect_pol<4>, grid, dim3(kBlock), lds,
                       stream, wf_a, wf_b, flags_a, flags_b, S, L, V, q4, G,
                       (unsigned)fscrunch, reverse ? 1 : 0,
                       pol_state == kPolStateIQUV ? 1 : 0, R, C,
                       (unsigned)tiles_r, out);
  SRTB_CHECK_LAUNCH();
  return hipSuccess;
}

size_t filterbank_stats_partials(size_t C) {
  return (size_t)kFilStatChunks * 2 * C;
}

hipError_t filterbank_channel_stats(const float* P, size_t R, size_t C,
                                    double* partials, float* mean,
                                    float* stddev, hipStream_t stream) {
  if (R == 0 || C == 0) return hipErrorInvalidValue;
  const int chunks = (int)(R < (size_t)kFilStatChunks ? R : kFilStatChunks);
  const uint32_t gx = (uint32_t)((C + kFilStatBlock - 1) / kFilStatBlock);
  hipLaunchKernelGGL(k_filterbank_stats_partial, dim3(gx, (uint32_t)chunks),
                     dim3(kFilStatBlock), 0, stream, P, R, C, chunks,
                     partials);
  hipLaunchKernelGGL(k_filterbank_stats_combine, dim3(gx),
                     dim3(kFilStatBlock), 0, stream, P, R, C, chunks,
                     partials, mean, stddev);
  SRTB_CHECK_LAUNCH();
  return hipSuccess;
}

hipError_t filterbank_quantize(const float* P, const float* mean,
                               const float* stddev, size_t R, size_t C,
                               uint8_t* out_u8, hipStream_t stream) {
  if (R == 0 || C == 0) return hipErrorInvalidValue;
  const size_t n = R * C;
  hipLaunchKernelGGL(k_filterbank_quantize, grid_for(n / 4), dim3(kBlock), 0,
                     stream, P, mean, stddev, n, C, out_u8);
  SRTB_CHECK_LAUNCH();
  return hipSuccess;
}

}  // namespace srtb_hip
