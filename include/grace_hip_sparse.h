/*
 * grace_hip_sparse.h — the threshold and random-k sparsifiers on bfloat16 gradients
 * (libgrace_hip.so, gfx950; grace_amd/csrc/sparse.hip and records.hip).
 *
 * A fifth header of the same library: the rules at the top of grace_hip.h hold for every entry
 * point here (device pointers, stream-ordered, nothing allocates or synchronises, grace_status_t,
 * f32 arithmetic as the reference's torch ops).  In addition:
 *   - a bfloat16 array travels as its 16-bit patterns, `uint16_t*`; any 2-byte alignment is
 *     accepted (16-byte aligned arrays take the vector paths, anything else the scalar loops);
 *   - a bf16 gradient is widened exactly: the residual, the workspace meta (bound, counts), the
 *     payload values and everything on the wire are f32 and bit for bit what the f32 entry point
 *     gives for the widened gradient, so f32 and bf16 ranks can share a wire and a name's state;
 *   - a bf16 dense result is the f32 result rounded once to nearest even, bit for bit torch's CPU
 *     `.to(torch.bfloat16)` (a NaN becomes 0x7FC0); at world > 1 the rounding comes after the
 *     rank-ordered sum from 0 and the division;
 *   - a null required pointer, a negative size or a size outside the stated limits returns
 *     GRACE_ERR_ARG with "<name>: ..." in grace_last_error() and launches nothing.
 */
#ifndef GRACE_HIP_SPARSE_H
#define GRACE_HIP_SPARSE_H

#include "grace_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* grace_threshold_step_w1 on a bfloat16 gradient: the same two launches, `residual` (modes 1, 2) and
 * the workspace's partials and meta f32 as the f32 form leaves them, `out` = bf16(0 + t | 0).  The
 * fix-up (max t < thr) never reads t back from the rounded `out`.
 * ws: grace_threshold_workspace_bytes(n). */
grace_status_t grace_threshold_step_w1_bf16(const uint16_t* g, float* residual, int32_t mode, float beta, float gamma,
                                            int64_t n, float thr, void* ws, uint16_t* out, void* stream);
/* t = beta r + gamma g with g bfloat16, t and r f32 (ResidualMemory.compensate); has_residual = 0:
 * t = g widened and r is not read.  t may be r.  n = 0 is GRACE_OK. */
grace_status_t grace_axpby_bf16(const float* r, const uint16_t* g, int32_t has_residual, float beta, float gamma,
                                float* t, int64_t n, void* stream);
/* grace_randomk_step_w1_dense on a bfloat16 gradient with a bfloat16 `out` written in full (no
 * recycled output, so no grouping buffers); `residual` f32, updated in place.  1 <= n <= 2^28.
 * ws: grace_randomk_step_w1_dense_workspace_bytes(n, k). */
grace_status_t grace_randomk_step_w1_dense_bf16(const uint16_t* g, float* residual, int32_t has_residual, float beta,
                                                float gamma, int64_t n, const int64_t* idx, int64_t k, uint16_t* out,
                                                void* ws, size_t ws_bytes, void* stream);
/* r[idx[j]] = vals[j] - vals[j] for the k drawn indices, vals = r[idx] gathered before (the residual
 * of a random-k step once its payload is taken: +0, NaN where the value is not finite).  An index
 * outside [0, n) is skipped.  k = 0 is GRACE_OK. */
grace_status_t grace_randomk_clear(const int64_t* idx, const float* vals, int64_t k, float* r, int64_t n, void* stream);
/* The world > 1 decode of random-k as a bfloat16 dense result: vals = `world` arrays of k f32 values
 * (rank-major), idx the k indices every rank drew alike;
 * out[idx[j]] = bf16((((0 + v0[j]) + v1[j]) + ...) / divisor), +0 elsewhere, all n elements written.
 * Duplicates of an index must carry equal values on every rank (they do when each rank gathered them
 * from one tensor).  An index outside [0, n) is skipped. */
grace_status_t grace_randomk_aggregate_bf16(const float* vals, const int64_t* idx, int64_t k, int32_t world,
                                            float divisor, uint16_t* out, int64_t n, void* stream);

/* Bytes of workspace grace_sparse_aggregate_padded_bf16 needs (0 for arguments it would refuse). */
size_t grace_sparse_aggregate_padded_bf16_workspace_bytes(int32_t world, int64_t n);
/* grace_sparse_aggregate_records_bf16 for the padded buffers of the threshold counts exchange: rank
 * w's block of 2 cap words at base + w 2 cap is {vals f32[cap] | idx i32[cap]} with no header, its
 * count is counts[w] (device int32[world]; the first min(max(count, 0), cap) entries are valid and
 * nothing past them is read), indices ascending within a rank.
 * out[i] = bf16((((0 + d0[i]) + d1[i]) + ...) / divisor), every one of the n elements written.
 * 1 <= cap <= n < 2^31, 1 <= world <= 1024.  An index outside [0, n) is skipped. */
grace_status_t grace_sparse_aggregate_padded_bf16(const uint32_t* base, int64_t cap, const int32_t* counts,
                                                  int32_t world, float divisor, uint16_t* out, int64_t n, void* ws,
                                                  size_t ws_bytes, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* GRACE_HIP_SPARSE_H */
