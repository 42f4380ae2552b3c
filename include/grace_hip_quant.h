/*
 * grace_hip_quant.h — QSGD and TernGrad on bfloat16 gradients
 * (libgrace_hip.so, gfx950; grace_amd/csrc/quant.hip).
 *
 * A third header of the same library: the rules at the top of grace_hip.h hold for every entry
 * point here (device pointers, stream-ordered, nothing allocates or synchronises, grace_status_t,
 * f32 arithmetic as the reference's torch ops).  In addition:
 *   - a bfloat16 array travels as its 16-bit patterns, `uint16_t*`, and must be 8-byte aligned;
 *   - a bf16 gradient is widened exactly: codes, bucket norms and TernGrad scalars are bit for bit
 *     what the f32 entry point writes for the widened gradient with the same seed, u, clip_in or
 *     norms_in.  The payload formats are the f32 ones, so f32 and bf16 ranks can share a wire;
 *   - a bf16 dense result is the f32 result rounded once to nearest even, bit for bit torch's CPU
 *     `.to(torch.bfloat16)` (a NaN becomes 0x7FC0); at world > 1 the rounding comes after the
 *     rank-ordered sum from 0 and the division;
 *   - each `_bf16` entry point has its f32 form's parameter list with only the gradient and / or the
 *     dense output turned into `uint16_t*`; the offset tables and the TernGrad workspace are the f32
 *     ones (grace_terngrad_workspace_bytes, seg_off / bkt_off / unit_off);
 *   - only the fast paths exist on bf16.  QSGD: bucket_size 128, nseg <= grace_qsgd_seg_max(),
 *     nbuckets < 2^24.  TernGrad: nseg <= grace_qsgd_seg_max(), n < 2^31.  Anything else, a null
 *     required pointer or a misaligned array returns GRACE_ERR_ARG with "<name>: ..." in
 *     grace_last_error() and launches nothing; an empty input is GRACE_OK with no launch.
 */
#ifndef GRACE_HIP_QUANT_H
#define GRACE_HIP_QUANT_H

#include "grace_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------------------------------------------------ QSGD */
/* grace_qsgd_compress_at on a bfloat16 gradient (x[0] is the bucket's element xoff; 0 for a whole
 * bucket): the codes (int8 for q < 128, fp16 otherwise) and f32 bucket norms of the widened values.
 * bucket_size must be 128. */
grace_status_t grace_qsgd_compress_at_bf16(const uint16_t* x, int64_t xoff, const int64_t* seg_off, const int64_t* bkt_off,
                                      int32_t nseg, int64_t nbuckets, int32_t quantum_num, int32_t bucket_size,
                                      int32_t variant, const float* u, uint64_t seed, const float* norms_in,
                                      float* norms_out, void* codes, void* stream);
/* grace_qsgd_step_w1 on a bfloat16 gradient: out = bf16(0 + (norm / q) * code) in one pass. */
grace_status_t grace_qsgd_step_w1_bf16(const uint16_t* x, const int64_t* seg_off, const int64_t* bkt_off, int32_t nseg,
                                  int64_t nbuckets, int32_t quantum_num, int32_t variant, const float* u,
                                  uint64_t seed, uint16_t* out, void* stream);
/* grace_qsgd_decompress with the result (after the rank-ordered sum and the division) rounded once
 * to bfloat16.  bucket_size must be 128 and n < 2^31. */
grace_status_t grace_qsgd_decompress_bf16(const void* codes, const float* norms, int64_t code_stride,
                                     int64_t norm_stride, int32_t world, const int64_t* seg_off,
                                     const int64_t* bkt_off, int32_t nseg, int64_t n, int32_t quantum_num,
                                     int32_t bucket_size, int32_t variant, int32_t aggregate, float divisor,
                                     uint16_t* out, void* stream);

/* -------------------------------------------------------------------------------------- TernGrad */
/* grace_terngrad_compress on a bfloat16 gradient: the int8 codes and f32 scalars of the widened
 * values (u, when given, 16-byte aligned). */
grace_status_t grace_terngrad_compress_bf16(const uint16_t* x, const int64_t* seg_off, const int64_t* unit_off,
                                       int32_t nseg, int64_t nunits, const float* clip_in, const float* u,
                                       uint64_t seed, int8_t* codes, float* scalars, void* ws,
                                       void* stream);
/* grace_terngrad_step_w1 on a bfloat16 gradient: the statistics pass, then one pass writing
 * out = bf16(0 + code * scalar); scalars[nseg] are still written. */
grace_status_t grace_terngrad_step_w1_bf16(const uint16_t* x, const int64_t* seg_off, const int64_t* unit_off, int32_t nseg,
                                     int64_t nunits, const float* clip_in, const float* u, uint64_t seed,
                                     float* scalars, void* ws, uint16_t* out, void* stream);
/* grace_terngrad_decompress with the result (after the rank-ordered sum and the division) rounded
 * once to bfloat16. */
grace_status_t grace_terngrad_decompress_bf16(const int8_t* codes, const float* scalars, int64_t code_stride,
                                         int64_t scal_stride, int32_t world, const int64_t* seg_off,
                                         int32_t nseg, int64_t n, int32_t aggregate, float divisor, uint16_t* out,
                                         void* stream);

#ifdef __cplusplus
}
#endif

#endif /* GRACE_HIP_QUANT_H */
