// The per-element functions of the element-wise codecs -- natural compression (both flavours), the
// fp16 round trip and one-bit's means and decode -- shared by the f32 kernels of quant.hip and
// elementwise.hip and the typed kernels of cast.hip: one copy, so a code or a decoded value cannot
// differ between a float32 and a bfloat16 gradient.
#pragma once

#include <hip/hip_fp16.h>

#include "common.h"

namespace grace {

// natural compression, cupy flavour (grace_dl/dist/compressor/natural.py:12-40): exponent
// rounded up when mantissa > randint(0, 2^23 - 1), clipped to [18, 145], code = sign | (E - 18).
__device__ __forceinline__ uint32_t natural_code(float xv, int32_t r) {
  const int32_t bits = __float_as_int(xv);
  const int32_t sign = bits & (int32_t)0x80000000;
  int32_t e = bits & 0x7F800000;
  const int32_t mant = bits & 0x007FFFFF;
  if (mant > r) e = (int32_t)((uint32_t)e + 0x00800000u);   // a NaN's exponent wraps, as the reference's int32 does
  e = min(max(e, (int32_t)0x09000000), (int32_t)0x48800000);
  return (uint32_t)(uint8_t)((sign >> 24) | ((e >> 23) - 18));
}

// device generator of the natural codec: one rand32 hash per quad plus xorshift32 steps
// (uniform01x4's stream), mapped onto [0, 0x7FFFFF) by a high multiply (the reference's randint
// range; the per-element 64-bit mixes and 64-bit modulo this replaced made the encoder ALU-bound)
__device__ __forceinline__ void natural_rand4(uint64_t seed, int64_t e, int32_t (&r)[4]) {
  uint32_t hq = rand32(seed, (uint64_t)e);
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    if (j) { hq = hq ? hq : 0x9E3779B9u; hq ^= hq << 13; hq ^= hq >> 17; hq ^= hq << 5; }
    r[j] = (int32_t)__umulhi(hq, 0x7FFFFFu);
  }
}

__device__ __forceinline__ float natural_dec(uint32_t c) {
  const uint32_t e = c & 0x7F;
  const float mag = __uint_as_float((e + 18u) << 23);
  const float v = c > 127 ? -mag : mag;
  return v * (e >= 1 ? 1.0f : 0.0f);   // 0x80 decodes to -0.0 as in the reference
}

// cnat_cuda flavour (cnat_cuda.cu:68-134): frexp mantissa m in [0.5, 1); exponent kept w.p.
// 2|m| - 1; LUT: biased E <= 17 -> 0, E -> E - 17 saturating at 127, +128 if negative.
__device__ __forceinline__ uint32_t cnat_code(float v, float r) {
  if (v == 0.f) return 0u;
  int ex;
  const float prob = fabsf(frexpf(v, &ex)) / 0.5f - 1.0f;
  if (r >= prob) ex -= 1;
  const int biased = ex + 127;
  int code = biased <= 17 ? 0 : min(biased - 17, 127);
  if (v < 0.f) code += 128;
  return (uint32_t)code;
}

__device__ __forceinline__ float cnat_dec(uint32_t c) {
  const uint32_t m = c & 0x7F;
  const uint32_t e = m == 0 ? 0u : m + 17u;
  return __uint_as_float(((c >> 7) << 31) | (e << 23));
}

// fp16 (grace_dl/dist/compressor/fp16.py): the payload's 16 bits (nearest even) and their value
__device__ __forceinline__ uint32_t f16_bits(float v) { return (uint32_t)__half_as_ushort(__float2half_rn(v)); }
__device__ __forceinline__ float f16_value(uint32_t h) { return __half2float(__ushort_as_half((unsigned short)h)); }

// The world-1 round trip of one element, out = 0 + decompress(compress(v)), by mode.
enum CastMode : int { kCastNatural = 0, kCastCnat = 1, kCastCnatDet = 2, kCastF16 = 3 };
template <int MODE>
__device__ __forceinline__ float cast_round_trip(float v, float u, int32_t ri) {
  if constexpr (MODE == kCastNatural) return 0.f + natural_dec(natural_code(v, ri));
  else if constexpr (MODE == kCastCnat || MODE == kCastCnatDet) return 0.f + cnat_dec(cnat_code(v, u));
  else return 0.f + __half2float(__float2half_rn(v));
}

// one-bit (grace_dl/dist/compressor/onebit.py:13-31).  The means from the three f64 sums
// (sum over x < 0, their count, sum over the rest, NaN included): each rounded to f32 first.
__device__ __forceinline__ void onebit_means(double sum0d, double num0d, double sum1d, int64_t n, float* out) {
  const float sum0 = (float)sum0d, num0 = (float)num0d, sum1 = (float)sum1d;
  const float num1 = (float)n - num0;
  out[0] = num0 > 0.f ? sum0 / num0 : sum0;
  out[1] = num1 > 0.f ? sum1 / num1 : sum1;
}
// decode: mask0 * mean0 + notmask * mean1, two products then the add (0 * inf stays NaN); quirk
// reproduces the dist flavour's uint8 `~` (notmask = 255 - mask0)
__device__ __forceinline__ float onebit_dec(uint32_t b, float m0, float m1, int quirk) {
  float nb = quirk ? (float)(255u - b) : (float)(1u - b);
  return (float)b * m0 + nb * m1;
}

}  // namespace grace
