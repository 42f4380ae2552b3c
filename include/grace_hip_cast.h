/*
 * grace_hip_cast.h — natural compression (both flavours), fp16 and one-bit on bfloat16 gradients,
 * and one-bit's fused step and W-rank decode for both element types
 * (libgrace_hip.so, gfx950; grace_amd/csrc/cast.hip).
 *
 * A sixth header of the same library: the rules at the top of grace_hip.h hold for every entry
 * point here (device pointers, stream-ordered, nothing allocates or synchronises, grace_status_t,
 * f32 arithmetic as the reference's torch ops).  In addition:
 *   - a bfloat16 array travels as its 16-bit patterns, `uint16_t*`; an odd address is refused;
 *   - a bf16 gradient is widened exactly; a bf16 dense result is the f32 result rounded once to
 *     nearest even, bit for bit torch's CPU `.to(torch.bfloat16)` (a NaN becomes 0x7FC0);
 *   - each `_bf16` entry point differs from its f32 form only in `uint16_t*` for the gradient and
 *     the dense output: the u8 codes, the f16 payload, mask0 and the means are the f32 entry
 *     point's for the widened gradient, bit for bit, under the same seed or injected randoms;
 *   - an argument error returns GRACE_ERR_ARG with "<name>: ..." in grace_last_error() and touches
 *     no device; n == 0 is GRACE_OK with no launch where n == 0 is accepted.
 * Every kernel handles 16 B of the gradient or the dense result per lane (8 bf16, 4 f32) when its
 * pointers allow it -- bf16 and f16 arrays and injected randoms 16-byte aligned, the codes of a bf16
 * kernel 8-byte, and at world > 1 a row stride that keeps every rank's row so aligned -- and guarded
 * per-element accesses otherwise and in the last, ragged group.  Nothing outside [0, n) is touched.
 */
#ifndef GRACE_HIP_CAST_H
#define GRACE_HIP_CAST_H

#include "grace_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------------------------- natural compression, fp16 */
/* grace_natural_compress_at on a bfloat16 tensor: the codes of the widened values.  The device
 * generator stays keyed per quad of four elements at xoff + the quad's first index (xoff a
 * multiple of 4). */
grace_status_t grace_natural_compress_at_bf16(const uint16_t* x, int64_t xoff, int64_t n, const int32_t* rand_int,
                                              uint64_t seed, uint8_t* codes, void* stream);
/* grace_cnat_compress_at on a bfloat16 tensor. */
grace_status_t grace_cnat_compress_at_bf16(const uint16_t* x, int64_t xoff, int64_t n, const float* rand,
                                           int32_t deterministic, uint64_t seed, uint8_t* codes, void* stream);
/* grace_fp16_compress on a bfloat16 tensor: f16(f32(x)), nearest even. */
grace_status_t grace_fp16_compress_bf16(const uint16_t* x, void* half_out, int64_t n, void* stream);
/* grace_cast_step_w1 from bfloat16 to bfloat16: out = bf16(0 + decompress(compress(f32(x)))), modes
 * 0 to 3 as there.  Unlike the f32 form it takes any 2-byte aligned x and out. */
grace_status_t grace_cast_step_w1_bf16(const uint16_t* x, int64_t n, int32_t mode, uint64_t seed, uint16_t* out,
                                       void* stream);
/* grace_natural_decompress with the result -- after the rank-ordered sum and the division, which
 * is skipped when divisor == 1 -- rounded once to bfloat16. */
grace_status_t grace_natural_decompress_bf16(const uint8_t* codes, int64_t stride, int32_t world, int64_t n,
                                             int32_t flavour, int32_t aggregate, float divisor, uint16_t* out,
                                             void* stream);
/* grace_fp16_decompress_aggregate with the quotient rounded once to bfloat16. */
grace_status_t grace_fp16_decompress_aggregate_bf16(const void* half_in, int64_t stride, int32_t world, int64_t n,
                                                    float divisor, uint16_t* out, void* stream);

/* ------------------------------------------------------------------------------------- one-bit */
/* Every one-bit entry point here takes ws of at least grace_reduce_workspace_bytes(n) bytes, 8-byte
 * aligned (f64 partial sums; it need not be zeroed and holds nothing between calls).  The three sums
 * (x over x < 0, their count, x over the rest: NaN is "not x < 0") are f64 over a partition and in
 * an order fixed by (n, the element type): the same bits on every call.  The means are
 *   sum0 = (float)S0, num0 = (float)N0, sum1 = (float)S1, num1 = (float)n - num0
 *   mean0 = num0 > 0 ? sum0 / num0 : sum0,  mean1 = num1 > 0 ? sum1 / num1 : sum1
 * and a decoded element is  dec = (float)b * mean0 + nb * mean1,  b = mask0, nb = 1 - b, or
 * 255 - b when quirk != 0 (two products, then the add: 0 * inf is NaN, not skipped). */

/* grace_onebit_encode on a bfloat16 tensor, in one pass over x plus a one-workgroup finish:
 * mask0 = (x < 0) as u8, means_dev[0..1]. */
grace_status_t grace_onebit_encode_bf16(const uint16_t* x, int64_t n, uint8_t* mask0, float* means_dev, void* ws,
                                        void* stream);
/* World-1 Allgather(OneBit, NoneMemory).step in two launches: means_dev[0..1] as above and
 * out = 0 + dec, the decode of this rank's own payload summed from 0 (the division by 1 is exact
 * and omitted). */
grace_status_t grace_onebit_step_w1(const float* x, int64_t n, int32_t quirk, float* means_dev, float* out, void* ws,
                                    void* stream);
grace_status_t grace_onebit_step_w1_bf16(const uint16_t* x, int64_t n, int32_t quirk, float* means_dev, uint16_t* out,
                                         void* ws, void* stream);
/* Decode + aggregate of `world` gathered payloads (rank w's mask0 at mask0_wn + w * n, its means at
 * mean0_w[w] and mean1_w[w]) in one launch: out = (((0 + dec_0) + dec_1) + ...) / divisor, summed
 * in rank order in f32; no division when divisor == 1. */
grace_status_t grace_onebit_decode_aggregate(const uint8_t* mask0_wn, const float* mean0_w, const float* mean1_w,
                                             int32_t world, int32_t quirk, float divisor, float* out, int64_t n,
                                             void* stream);
grace_status_t grace_onebit_decode_aggregate_bf16(const uint8_t* mask0_wn, const float* mean0_w, const float* mean1_w,
                                                  int32_t world, int32_t quirk, float divisor, uint16_t* out, int64_t n,
                                                  void* stream);

#ifdef __cplusplus
}
#endif

#endif /* GRACE_HIP_CAST_H */
