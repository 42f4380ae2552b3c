/*
 * grace_hip_sketch.h — quantile-bucket quantisation (SketchML: Jiang et al., "SketchML: Accelerating
 * Distributed Machine Learning with Data Sketches", SIGMOD 2018) on float32 and bfloat16 gradients
 * (libgrace_hip.so, gfx950; grace_amd/csrc/sketch.hip).
 *
 * An eighth header of the same library: the rules at the top of grace_hip.h hold for every entry
 * point here (device pointers, stream-ordered, nothing allocates or synchronises, grace_status_t,
 * f32 arithmetic with every operation rounded on its own).  In addition:
 *   - a bfloat16 array travels as its 16-bit patterns, `uint16_t*`; an odd address is refused;
 *   - a bf16 gradient is widened exactly; a bf16 dense result is the f32 result rounded once to
 *     nearest even (a NaN becomes 0x7FC0);
 *   - each `_bf16` entry point differs from its f32 form only in `uint16_t*` for the gradient or the
 *     dense result: edges, codes and means are the f32 entry point's for the widened gradient;
 *   - an argument error returns GRACE_ERR_ARG with "<name>: ..." in grace_last_error() and touches
 *     no device; n == 0 is GRACE_OK with no launch.
 *
 * x has n elements, 1 <= n < 2^31; q is the number of buckets, 2 <= q <= 256.
 *
 * Order: numeric f32 order.  A zero of either sign counts as +0.0 everywhere, in the edges and in
 * the search; +-Inf are ordinary values.  NaN gradients are outside the contract: the result is
 * unspecified, but nothing outside the arrays is touched and every kernel makes a fixed number of
 * passes.
 *
 * Edges: edges[j] = sorted(x)[floor(j * (n - 1) / q)] for j = 0 .. q, the product taken in 64-bit
 * integers.  They are exact order statistics, so every edge is an element of x (a zero is +0.0), and
 * they are the same bits on every call: they come from integer counts alone.
 * Code:  code_i = #{ j in 1 .. q-1 : edges[j] <= x_i }, in [0, q-1].  Repeated edges leave buckets
 * empty.
 * Means: means[b] = the sum of the elements with code b, taken in f64, divided in f64 by their
 * number and rounded once to f32; 0 for an empty bucket.  The order of the f64 sum is NOT fixed
 * (atomic adds inside and across workgroups): two calls on the same x may differ in the last bit of
 * a mean.  Every order stays within 2^-52 * sum|x_i| of the exact sum.
 * Decode: d_i = means[code_i] (a code above q - 1, which no encoder here writes, decodes as q - 1).
 *
 * Wire: codes u8[n] when q > 16; u8[ceil(n / 2)] when q <= 16, element 2i in the low nibble and the
 * unused high nibble of an odd n zero; means f32[q].
 *
 * The vector paths (16 B of the gradient or the dense result per lane, one packed store or load of
 * the lane's codes) run when the gradient and the dense result are 16-byte aligned and the codes
 * (every rank's row, at world > 1) 8-byte aligned; guarded per-element accesses run otherwise and in
 * the ragged tail, inside the same kernels.  Nothing outside [0, n), or [0, ceil(n / 2)) of packed
 * codes, is touched.
 *
 * ws: grace_sketch_workspace_bytes(n, q) bytes, 8-byte aligned.  No condition on entry: every call
 * zeroes the counters it uses with a kernel of its own before its first pass, and no condition holds
 * on exit.  Calls that share a ws share a stream.
 */
#ifndef GRACE_HIP_SKETCH_H
#define GRACE_HIP_SKETCH_H

#include "grace_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Bytes of workspace of every call below on n elements and q buckets (0 for arguments they refuse). */
size_t grace_sketch_workspace_bytes(int64_t n, int32_t q);

/* The multi-select alone: edges[q + 1].  Four passes over an f32 x, two over a bf16 x. */
grace_status_t grace_sketch_edges(const float* x, int64_t n, int32_t q, float* edges, void* ws, void* stream);
grace_status_t grace_sketch_edges_bf16(const uint16_t* x, int64_t n, int32_t q, float* edges, void* ws,
                                       void* stream);
/* means[q] and the codes of x (the wire above): the select, then one pass that searches, sums and packs. */
grace_status_t grace_sketch_compress(const float* x, int64_t n, int32_t q, float* means, uint8_t* codes, void* ws,
                                     void* stream);
grace_status_t grace_sketch_compress_bf16(const uint16_t* x, int64_t n, int32_t q, float* means, uint8_t* codes,
                                          void* ws, void* stream);
/* World-1 Allgather(Sketch, NoneMemory).step: means[q] as above and out = 0 + d in the gradient's type.
 * The codes are kept in ws between the encode pass and the decode pass. */
grace_status_t grace_sketch_step_w1(const float* x, int64_t n, int32_t q, float* means, float* out, void* ws,
                                    void* stream);
grace_status_t grace_sketch_step_w1_bf16(const uint16_t* x, int64_t n, int32_t q, float* means, uint16_t* out,
                                         void* ws, void* stream);
/* Decode + aggregate of `world` (1 to 1024) gathered payloads in one launch: rank w's codes at
 * codes + w * code_stride_bytes (at least a row, n or ceil(n / 2) bytes, when world > 1), its means
 * at means + w * q; out = (((0 + d_0) + d_1) + ...) / divisor, summed in rank order in f32; no
 * division when divisor == 1. */
grace_status_t grace_sketch_decode_aggregate(const uint8_t* codes, int64_t code_stride_bytes, const float* means,
                                             int32_t world, int64_t n, int32_t q, float divisor, float* out,
                                             void* stream);
grace_status_t grace_sketch_decode_aggregate_bf16(const uint8_t* codes, int64_t code_stride_bytes,
                                                  const float* means, int32_t world, int64_t n, int32_t q,
                                                  float divisor, uint16_t* out, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* GRACE_HIP_SKETCH_H */
