/*
 * grace_hip_sign.h — the sign family on bfloat16 gradients and the fused EF-signSGD step
 * (libgrace_hip.so, gfx950; grace_amd/csrc/sign.hip).
 *
 * A second header of the same library: the rules at the top of grace_hip.h hold for every entry
 * point here (device pointers, stream-ordered, nothing allocates or synchronises, grace_status_t,
 * f32 arithmetic as the reference's torch ops).  In addition:
 *   - a bfloat16 array travels as its 16-bit patterns, `uint16_t*`; an odd address is refused;
 *   - a bf16 gradient is widened exactly; a bf16 dense result is the f32 result rounded once to
 *     nearest even, bit for bit torch's CPU `.to(torch.bfloat16)` (a NaN becomes 0x7FC0);
 *   - each `_bf16` entry point differs from its f32 form only in `uint16_t*` for the gradient and
 *     the dense output; everything else (residual, momentum, mean, codes, words) is identical;
 *   - an argument error returns GRACE_ERR_ARG with "<name>: ..." in grace_last_error() and touches
 *     no device; n == 0 is GRACE_OK with no launch.
 * Every kernel takes a vector path when its pointers allow it (bf16 arrays 8-byte aligned, f32
 * arrays 16-byte, codes 4-byte, and at world > 1 n % 4 == 0) and a guarded scalar path otherwise.
 */
#ifndef GRACE_HIP_SIGN_H
#define GRACE_HIP_SIGN_H

#include "grace_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ----------------------------------------------------------------------------------- EF-signSGD */
/* Bytes of workspace grace_efsign_step needs for a bucket of n elements (the f64 partial sums of
 * pass A; it need not be zeroed and holds nothing between calls). */
size_t grace_efsign_workspace_bytes(int64_t n);

/* One EF-signSGD step of one rank (grace_dl/dist/memory/efsignsgd.py:9-19 and
 * compressor/efsignsgd.py:12-33) in two launches:
 *   t        = has_residual ? residual + lr_mem * g : g          (two roundings, no contraction)
 *   mean     = (float)sum|t| / (float)n     sum in f64 over a fixed partition in a fixed order:
 *                                           the same bits on every call with the same arguments
 *   code     = (t >= 0)                     (-0 -> 1, NaN -> 0)
 *   dec      = mean * ((float)code * 2 - 1)
 *   residual = t - dec                      written in place (read only when has_residual != 0)
 *   out      = (0.f + dec) / lr_agg         the world-1 dense result, IEEE division
 * mean_out receives the mean (f32[1]).  codes (u8[n]) and out may each be NULL and are then not
 * written.  g is never written.  ws: at least grace_efsign_workspace_bytes(n) bytes. */
grace_status_t grace_efsign_step(const float* g, float* residual, int32_t has_residual, float lr_mem, int64_t n,
                                 float* mean_out, uint8_t* codes, float* out, float lr_agg, void* ws, size_t ws_bytes,
                                 void* stream);
/* The same step on a bfloat16 gradient; the residual and the mean stay f32, out is bf16. */
grace_status_t grace_efsign_step_bf16(const uint16_t* g, float* residual, int32_t has_residual, float lr_mem, int64_t n,
                                      float* mean_out, uint8_t* codes, uint16_t* out, float lr_agg, void* ws,
                                      size_t ws_bytes, void* stream);

/* Decode + aggregate of `world` gathered EF-signSGD payloads (means f32[world], rank w's codes at
 * codes_wn + w * n) in one launch: out = (((0 + m_0 d_0) + m_1 d_1) + ...) / lr_agg with
 * d_w = (float)code_w * 2 - 1, summed in rank order in f32, not averaged. */
grace_status_t grace_efsign_decode_aggregate(const float* means, const uint8_t* codes_wn, int32_t world, float lr_agg,
                                             float* out, int64_t n, void* stream);
/* The same with the quotient rounded once to bfloat16. */
grace_status_t grace_efsign_decode_aggregate_bf16(const float* means, const uint8_t* codes_wn, int32_t world,
                                                  float lr_agg, uint16_t* out, int64_t n, void* stream);

/* ------------------------------------------------------------------------ signSGD and Signum */
/* grace_sign_encode on a bfloat16 tensor: the codes of the widened values. */
grace_status_t grace_sign_encode_bf16(const uint16_t* x, uint8_t* codes, int64_t n, void* stream);
/* grace_sign_encode_bits on a bfloat16 tensor: the same 1-bit words. */
grace_status_t grace_sign_encode_bits_bf16(const uint16_t* x, int64_t n, uint32_t* words, void* stream);
/* grace_sign_step_w1 on a bfloat16 tensor: out = +-1 as bf16 (0x3F80 / 0xBF80); codes may be NULL. */
grace_status_t grace_sign_step_w1_bf16(const uint16_t* x, uint8_t* codes, uint16_t* out, int64_t n, void* stream);
/* grace_sign_majority with the vote written as bf16 +-1. */
grace_status_t grace_sign_majority_bf16(const uint8_t* codes_wn, int32_t world, uint16_t* out, int64_t n,
                                        void* stream);
/* grace_sign_majority_bits with the vote written as bf16 +-1 (world <= 63). */
grace_status_t grace_sign_majority_bits_bf16(const uint32_t* words, int64_t stride_words, int32_t world, int64_t n,
                                             uint16_t* out, void* stream);
/* grace_signum_encode on a bfloat16 gradient; the momentum buffer stays f32 and receives the bits
 * the f32 entry point gives for the widened gradient. */
grace_status_t grace_signum_encode_bf16(const uint16_t* g, float* momentum, int32_t has_prev, float coef_g,
                                        float coef_m, uint8_t* codes, int64_t n, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* GRACE_HIP_SIGN_H */
