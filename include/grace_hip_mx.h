/*
 * grace_hip_mx.h — the OCP Microscaling (MX) formats as a gradient codec on float32 and bfloat16
 * gradients: blocks of 32 elements that share one E8M0 power-of-two scale, elements in FP8 (E4M3, E5M2),
 * FP6 (E2M3, E3M2) or FP4 (E2M1); 8.25, 6.25 or 4.25 bits an element (libgrace_hip.so, gfx950;
 * grace_amd/csrc/mx.hip).
 *
 * An eleventh header of the same library: the rules at the top of grace_hip.h hold for every entry
 * point here (device pointers, stream-ordered, nothing allocates or synchronises, grace_status_t).
 * In addition:
 *   - a bfloat16 array travels as its 16-bit patterns, `uint16_t*`; an odd address is refused;
 *   - a bf16 gradient is widened exactly; a bf16 dense result is the f32 result rounded once to nearest
 *     even (a NaN becomes 0x7FC0);
 *   - each `_bf16` entry point differs from its f32 form only in `uint16_t*` for the gradient or the
 *     dense result: the payload is the f32 entry point's for the widened gradient;
 *   - an argument error (n outside [0, 2^31), a format outside 0..4, a rounding outside 0..1, a null or
 *     misaligned pointer, world outside [1, 1024], a zero divisor, a stride that is no multiple of 16 or
 *     shorter than the payload) returns GRACE_ERR_ARG with "<name>: ..." in the last-error string and
 *     touches no device; n == 0 is GRACE_OK with no launch.
 *
 * Blocks.  Block b holds elements 32 b .. 32 b + 31 of the flat tensor; nb = ceil(n / 32).  Positions
 * past n in the last block count as +0: they do not raise the maximum and their codes are 0.
 *
 * Formats.  An element code is sign | exponent field | mantissa field, `bits` wide.
 *
 *   format  name       bits  exponent  mantissa  bias  emax  max normal  largest code   Inf / NaN codes
 *   0       fp8_e4m3   8     4         3         7     8     448         0x7E           S.1111.111 is NaN
 *   1       fp8_e5m2   8     5         2         15    15    57344       0x7B           S.11111.00 Inf, else NaN
 *   2       fp6_e2m3   6     2         3         1     2     7.5         0x1F           none
 *   3       fp6_e3m2   6     3         2         3     4     28          0x1F           none
 *   4       fp4_e2m1   4     2         1         1     2     6           0x7            none
 *
 * With ce the exponent field, cm the mantissa field and M the mantissa width, a magnitude code stands for
 * (2^M + cm) 2^(ce - bias - M) when ce > 0 and for cm 2^(1 - bias - M) when ce == 0 (subnormals, all five
 * formats have them).  The values grow with the magnitude code, so neighbouring codes are neighbouring
 * values.  The encoder never emits a code above `largest code`, so never an Inf or a NaN element.
 *
 * Scale.  A = the largest magnitude bit pattern of the block (the f32 bits without the sign; a NaN is
 * above Inf).  If A >= 0x7F800000 the scale byte is 255, all 32 codes are 0 and the block decodes to NaN
 * (0x7FC00000).  Otherwise, with E = A >> 23 (0 for a denormal or zero maximum), the scale byte is
 * e = clamp(E - emax, 0, 254) and the scale is X = 2^(e - 127): the OCP specification's floor rule.
 *
 * Element.  y = |x| / X as a real number; y above the max normal counts as the max normal; the code's sign
 * bit is x's, so -0 keeps its sign.  With lo the largest representable value <= y and hi the next one up:
 *   rounding 0, nearest     the nearer of lo and hi, a tie to the one whose code is even;
 *   rounding 1, stochastic  hi iff u < (y - lo) / (hi - lo), evaluated exactly; y >= max normal stays.
 * u is a 24-bit uniform k / 2^24, k in 0 .. 2^24 - 1.  With `u` null, element i draws lane i & 3 of the
 * library's four-uniform generator at (seed, 4 (i / 4)) (common.h uniform01x4; the bucket codecs draw
 * the same way).  With `u` given, u[i] is read instead and k = floor(u[i] 2^24) clamped to that range,
 * so an array of the generator's own values reproduces the seeded call byte for byte.
 *
 * The device evaluates all of this on the 24-bit significand of x as an integer (a denormal x is
 * normalised first), so nothing is lost where x / X would fall below the f32 normal range: lo is a
 * right shift, y - lo the bits shifted out, and both roundings compare integers.
 *
 * Decode.  code -> +-value(code) 2^(e - 127) as f32; scale byte 255 gives NaN; an Inf or NaN element
 * code of a hand-made payload gives Inf or NaN.  The product is exact for every payload the encoder
 * writes: value(code) has at most 4 significant bits and is a multiple of 2^(1 - bias - M) >= 2^-16, so
 * the product is a multiple of 2^-143 (representable, if need be as an f32 denormal) with at most 4
 * significant bits; and e <= E - emax with value <= max normal <= (2 - 2^-3) 2^emax keeps it at or below
 * (2 - 2^-3) 2^(E - 127) with E <= 254, which is finite.  A hand-made payload can overflow to Inf.
 *
 * Aggregate.  out = ((d^0 + d^1) + ...) in f32 in rank order (world 1: d^0 itself, so -0 stays -0); one
 * division unless the divisor is 1; a bf16 result gets one rounding to nearest even.
 *
 * The wire, one uint8 buffer, the same for a float32 and a bfloat16 gradient:
 *   scales   nb bytes, zero-padded to a multiple of 16;
 *   codes    block after block, 4 `bits` bytes a block, a little-endian bit stream in which element j of
 *            the block occupies bits j `bits` .. j `bits` + `bits` - 1 (FP8: element j is byte j; FP4:
 *            element 2j is the low nibble of byte j); zero-padded to a multiple of 16.
 * Every byte is written, padding included, so equal inputs give equal bytes.
 *
 * The vector paths (16 B of the gradient or the dense result per access) run when that array is 16-byte
 * aligned; guarded per-element accesses run otherwise and in the ragged last chunk, inside the same
 * kernels.  Nothing outside [0, n) of a gradient, of `u` or of a result is touched, nothing outside the
 * payload's size written and nothing outside [0, stride_bytes) of a payload read.
 */
#ifndef GRACE_HIP_MX_H
#define GRACE_HIP_MX_H

#include "grace_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The payload's length in bytes: ceil16(nb) + ceil16(4 bits nb).  0 for n outside [1, 2^31) or a format
 * outside 0..4. */
size_t grace_mx_payload_bytes(int64_t n, int32_t format);

/* payload (that many bytes, 16-byte aligned) = the wire above; x is read once.  u: null, or n floats. */
grace_status_t grace_mx_compress(const float* x, int64_t n, int32_t format, int32_t rounding, uint64_t seed,
                                 const float* u, uint8_t* payload, void* stream);
grace_status_t grace_mx_compress_bf16(const uint16_t* x, int64_t n, int32_t format, int32_t rounding, uint64_t seed,
                                      const float* u, uint8_t* payload, void* stream);
/* World-1 Allgather(MX, NoneMemory).step: out = decode(encode(x)) elementwise in the gradient's type, from
 * the registers the codes were made in; neither codes nor scales reach memory. */
grace_status_t grace_mx_step_w1(const float* x, int64_t n, int32_t format, int32_t rounding, uint64_t seed,
                                const float* u, float* out, void* stream);
grace_status_t grace_mx_step_w1_bf16(const uint16_t* x, int64_t n, int32_t format, int32_t rounding, uint64_t seed,
                                     const float* u, uint16_t* out, void* stream);
/* Decode + aggregate of `world` (1 to 1024) gathered payloads in one launch: rank w's payload starts at
 * payloads + w * stride_bytes (16-byte aligned; stride_bytes a multiple of 16 and at least the payload of
 * (n, format)); out = the rank-ordered f32 sum / divisor; no division when divisor == 1. */
grace_status_t grace_mx_decode_aggregate(const uint8_t* payloads, int64_t stride_bytes, int32_t world, int64_t n,
                                         int32_t format, float divisor, float* out, void* stream);
grace_status_t grace_mx_decode_aggregate_bf16(const uint8_t* payloads, int64_t stride_bytes, int32_t world, int64_t n,
                                              int32_t format, float divisor, uint16_t* out, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* GRACE_HIP_MX_H */
