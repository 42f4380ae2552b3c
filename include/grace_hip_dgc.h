/*
 * grace_hip_dgc.h — Deep Gradient Compression on bfloat16 gradients
 * (libgrace_hip.so, gfx950; grace_amd/csrc/dgc.hip and records.hip).
 *
 * A fourth header of the same library: the rules at the top of grace_hip.h hold for every entry
 * point here (device pointers, stream-ordered, nothing allocates or synchronises, grace_status_t,
 * f32 arithmetic as the reference's torch ops).  In addition:
 *   - a bfloat16 array travels as its 16-bit patterns, `uint16_t*`; any 2-byte alignment is
 *     accepted (8-byte aligned arrays beside 16-byte aligned f32 ones take the vector path);
 *   - a bf16 gradient is widened exactly: the momentum state (residual, accum), the thresholds,
 *     the counts and the records on the wire are f32 and bit for bit what the f32 entry point gives
 *     for the widened gradient, so f32 and bf16 ranks can share a wire and a name's state;
 *   - a bf16 dense result is the f32 result rounded once to nearest even, bit for bit torch's CPU
 *     `.to(torch.bfloat16)` (a NaN becomes 0x7FC0); at world > 1 the rounding comes after the
 *     rank-ordered sum from 0 and the division;
 *   - each `_bf16` twin has its f32 form's parameter list with only the gradient and / or the dense
 *     output turned into `uint16_t*`, and uses the f32 form's workspace;
 *   - a null required pointer, a negative size or new state that aliases the old returns
 *     GRACE_ERR_ARG with "<name>: ..." in grace_last_error() and launches nothing.
 */
#ifndef GRACE_HIP_DGC_H
#define GRACE_HIP_DGC_H

#include "grace_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* grace_dgc_step_w1_fused on a bfloat16 gradient: the same launches from the old f32 state into
 * new f32 buffers, `out` = bf16(result).  ws: grace_dgc_step_w1_fused_workspace_bytes(n). */
grace_status_t grace_dgc_step_w1_fused_bf16(const uint16_t* g, const float* residual, const float* accum, int32_t has_state,
                                       float momentum, int64_t n, const float* top_vals, int64_t ks, double ratio,
                                       void* ws, float* residual_out, float* accum_out, uint16_t* out, void* stream);
/* grace_dgc_sample_comp on a bfloat16 gradient: |compensated t| at the sample indices, f32. */
grace_status_t grace_dgc_sample_comp_bf16(const uint16_t* g, const float* residual, const float* accum, int32_t has_state,
                                     float momentum, int64_t n, const int64_t* sample_idx, uint64_t seed, int64_t ns,
                                     float* sample_abs, void* stream);
/* grace_dgc_compensate on a bfloat16 gradient: r = m r + g, a = a + r in place (f32). */
grace_status_t grace_dgc_compensate_bf16(const uint16_t* g, float* residual, float* accum, int32_t has_state,
                                    float momentum, int64_t n, void* stream);
/* grace_dgc_step_w1 (mask the f32 memory at ws's final threshold) with out = bf16(0 + t | 0). */
grace_status_t grace_dgc_step_w1_bf16(const float* t, float* residual, float* accum, int64_t n, const void* ws, uint16_t* out,
                                 void* stream);
/* grace_sumsq of a bfloat16 tensor: bit for bit grace_sumsq of the widened tensor (same grid, same
 * per-thread order).  ws: grace_sumsq_workspace_bytes(). */
grace_status_t grace_sumsq_bf16(const uint16_t* x, int64_t n, void* ws, float* out_dev, void* stream);
/* grace_clip_by_sumsq of a bfloat16 tensor; the result is f32 (the bound sqrt(s / world) is not a
 * bfloat16 number). */
grace_status_t grace_clip_by_sumsq_bf16(const uint16_t* x, const float* sumsq_dev, float world, float* out, int64_t n,
                                   void* stream);

/* Bytes of workspace grace_sparse_aggregate_records_bf16 needs (0 for arguments it would refuse). */
size_t grace_sparse_aggregate_records_bf16_workspace_bytes(int32_t world, int64_t n);
/* Rank-ordered aggregate of `world` gathered capacity-bounded records ({count, cap, 0, 0 | vals
 * f32[cap] | idx i32[cap]}, `stride` = grace_exchange_record_words(cap) words apart, indices
 * ascending within a rank, the first min(count, cap) entries valid) as a bfloat16 dense result:
 * out[i] = bf16((((0 + d0[i]) + d1[i]) + ...) / divisor), every one of the n elements written in one
 * pass over the output; stat = {max count, max count > cap} as grace_sparse_aggregate_capped sets
 * it.  1 <= cap <= n < 2^31, 1 <= world <= 1024.  An index outside [0, n) is skipped. */
grace_status_t grace_sparse_aggregate_records_bf16(const uint32_t* recs, int64_t stride, int64_t cap, int32_t world,
                                              float divisor, uint16_t* out, int64_t n, uint32_t* stat, void* ws,
                                              size_t ws_bytes, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* GRACE_HIP_DGC_H */
