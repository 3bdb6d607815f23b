// Shared device helpers for srtb_amd HIP kernels (gfx950, wave64).
#pragma once

#include <hip/hip_runtime.h>
#include <cstddef>
#include <cstdint>

namespace srtb_hip {

constexpr int kBlock = 256;          // multiple of wave64
constexpr int kMaxBlocks = 4096;     // grid-stride cap (G11: ~256 CU * 8-16)

inline dim3 grid_for(size_t n, int block = kBlock, int cap = kMaxBlocks) {
  size_t b = (n + block - 1) / block;
  if (b > static_cast<size_t>(cap)) b = cap;
  if (b == 0) b = 1;
  return dim3(static_cast<uint32_t>(b));
}

#define SRTB_CHECK_LAUNCH()                        \
  do {                                             \
    hipError_t err_ = hipGetLastError();           \
    if (err_ != hipSuccess) return err_;           \
  } while (0)

// ---- wave64 + block reductions (fp32 lanes, fp64 block output) ----

__device__ inline float wave_reduce_sum(float v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
  return v;
}

__device__ inline double wave_reduce_sum(double v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
  return v;
}

// Block-level sum over kBlock threads; returns valid value on thread 0.
template <typename T>
__device__ inline T block_reduce_sum(T v) {
  __shared__ T lds[kBlock / 64];
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  v = wave_reduce_sum(v);
  if (lane == 0) lds[wave] = v;
  __syncthreads();
  T out = T(0);
  if (wave == 0) {
    out = (lane < kBlock / 64) ? lds[lane] : T(0);
    out = wave_reduce_sum(out);
  }
  __syncthreads();
  return out;
}

__device__ inline float norm2(float2 c) { return c.x * c.x + c.y * c.y; }

// Coherent-dedispersion phase factor (reference phase_factor_v3,
// coherent_dedispersion.hpp:133-150): k = D*1e6*dm/f*((f-f_c)/f_c)^2 with
// |k| up to ~1e9, so everything before the wrap stays in fp64.
constexpr double kDispersionConstantMHz = 4.148808e3;

__device__ inline float2 srtb_dedisp_factor(size_t i, double f_min,
                                            double f_c, double df,
                                            double dm) {
  const double f = f_min + df * (double)i;
  const double r = (f - f_c) / f_c;
  const double k = (kDispersionConstantMHz * 1e6) * dm / f * (r * r);
  double k_int;
  const double k_frac = modf(k, &k_int);
  // |k| reaches ~1e9 so the reduction above must be fp64, but the wrapped
  // phase is in (-2pi, 2pi): fast f32 sincos is accurate to ~1.5e-6 rad
  // here, comparable to the fp32 storage precision, at a fraction of the
  // fp64 sincos VALU cost.
  const float phi = (float)(-2.0 * M_PI * k_frac);
  float s, c;
  __sincosf(phi, &s, &c);
  return make_float2(c, s);
}

// Column-polynomial form of the same factor for the bins of one FFT column,
// f_j = f0 + j*delta (f0 = f_min + df*bin0, delta = df*stride).  The turn
// count k(f) = A (f-f_c)^2 / f, A = D*1e6*dm/f_c^2, expands about f0 as
//   k(f_j) = c0 + c1 j + c2 j^2 + c3 j^3 + O(A f_c^2 delta^4 j^4 / f0^5)
// with, writing q = D*1e6*dm/f0, r = (f0-f_c)/f_c, u = delta/f0:
//   c0 = q r^2   c1 = q r (r+2) u   c2 = q u^2   c3 = -q u^3
// (no cancellation in any coefficient).  Only frac(k) matters, so each
// coefficient's fraction is held as a 64-bit fixed-point turn count and the
// cubic is combined in wrapping integer arithmetic: the ~1e6-turn integer
// parts vanish exactly and no per-bin fp64 division, modf or range reduction
// is left.  The caller (fft_col_pass) checks the truncation bound on the host
// and falls back to srtb_dedisp_factor when it does not hold.
struct DedispPoly {
  unsigned long long c0, c1, c2, c3;  // frac(c_p) * 2^64
};

__device__ inline unsigned long long srtb_turns_to_fix64(double t) {
  const double fr = t - floor(t);  // [0, 1]; 1.0 only for tiny negative t
  return fr < 1.0 ? (unsigned long long)(fr * 18446744073709551616.0) : 0ull;
}

// per-thread set-up: three fp64 divisions for a whole column
__device__ inline DedispPoly srtb_dedisp_poly_setup(unsigned long long bin0,
                                                    unsigned long long stride,
                                                    double f_min, double f_c,
                                                    double df, double dm) {
  const double f0 = f_min + df * (double)bin0;
  const double r = (f0 - f_c) / f_c;
  const double q = (kDispersionConstantMHz * 1e6) * dm / f0;
  const double u = df * (double)stride / f0;
  DedispPoly p;
  p.c0 = srtb_turns_to_fix64(q * (r * r));  // srtb_dedisp_factor's k at bin0
  p.c1 = srtb_turns_to_fix64(q * r * (r + 2.0) * u);
  p.c2 = srtb_turns_to_fix64(q * (u * u));
  p.c3 = srtb_turns_to_fix64(-q * (u * u) * u);
  return p;
}

// exp(-2 pi i frac(k(f_j))); j must be a compile-time constant at the call
// site (fully unrolled loops) so the integer multiplies fold to immediates.
// The top 32 bits of the wrapped sum are a signed turn count in [-0.5, 0.5),
// which the hardware sine/cosine take directly (their argument is in turns).
__device__ __forceinline__ float2 srtb_dedisp_poly_eval(const DedispPoly& p,
                                                        unsigned j) {
  const unsigned long long jj = j;
  const unsigned long long t = p.c0 + jj * (p.c1 + jj * (p.c2 + jj * p.c3));
  const float turns = (float)(int)(unsigned)(t >> 32) * 0x1p-32f;
  return make_float2(__builtin_amdgcn_cosf(turns),
                     -__builtin_amdgcn_sinf(turns));
}

}  // namespace srtb_hip
