/*
 * grace_hip_u8bit.h — 8-bit codebook quantisation with one absmax scale per block of the tensor or
 * per tensor (Dettmers, "8-Bit Approximations for Parallelism in Deep Learning", arXiv:1511.04561),
 * on float32 and bfloat16 gradients (libgrace_hip.so, gfx950; grace_amd/csrc/u8bit.hip, DESIGN.md
 * section 15).
 *
 * A seventh header of the same library: the rules at the top of grace_hip.h hold for every entry
 * point here (device pointers, stream-ordered, nothing allocates or synchronises, grace_status_t,
 * f32 arithmetic with every operation rounded on its own).  In addition:
 *   - a bfloat16 array travels as its 16-bit patterns, `uint16_t*`; an odd address is refused;
 *   - a bf16 gradient is widened exactly; a bf16 dense result is the f32 result rounded once to
 *     nearest even (a NaN becomes 0x7FC0);
 *   - each `_bf16` entry point differs from its f32 form only in `uint16_t*` for the gradient and
 *     the dense result: the codes and the scales are the f32 entry point's for the widened
 *     gradient, bit for bit;
 *   - an argument error returns GRACE_ERR_ARG with "<name>: ..." in grace_last_error() and touches
 *     no device; n == 0 is GRACE_OK with no launch.
 *
 * Tables: `edges` and `values` are 128 f32 each on the device, ascending, first entry >= 0.  That
 * is a precondition: the host cannot see a device table.
 *
 * block: 0 (one scale for the whole tensor) or a power of two from 256 to 4096.  Blocks are counted
 * from element 0 whatever the pointer's alignment, the last one may be short, and
 * nblk = block ? ceil(n / block) : 1.
 *
 * Encode, per block, in f32:
 *   a = max |x_i| with NaN elements ignored (0 for an all-NaN block); scales[b] = a
 *   y = |x_i| / a          (IEEE division; 0/0, inf/inf and a NaN element give a NaN y)
 *   i = max(0, #{j : edges[j] <= y} - 1), in [0, 127]; a NaN y counts nothing
 *   code_i = x_i < 0 ? -i : i, an int8
 * Decode: d = 0 when code == 0, else values[|code|] * a (one f32 multiply) with the sign of code.
 * (-128 is not a code; it decodes as -values[0] * a.)
 *
 * The vector paths (16 B of the gradient or the dense result per lane, 4 or 8 codes per store) run
 * when the gradient and the dense result are 16-byte aligned, the codes 4-byte (f32) or 8-byte
 * (bf16) and, at world > 1, code_stride keeps every rank's row so aligned; guarded per-element
 * accesses run otherwise and in the ragged tail.  Nothing outside [0, n) is touched.
 *
 * ws: grace_reduce_workspace_bytes(n) bytes, 4-byte aligned, used (and required) only when
 * block == 0.  Its first four bytes are the arrival counter of the tensor-wide maximum: zero on
 * entry, zero again when the call's kernels have run.  Calls that share a ws share a stream.
 */
#ifndef GRACE_HIP_U8BIT_H
#define GRACE_HIP_U8BIT_H

#include "grace_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* codes[n] and scales[nblk] of x.  Block-wise it is one launch that reads x once; tensor-wide it is
 * a maximum pass and the encode pass. */
grace_status_t grace_u8bit_compress(const float* x, int64_t n, int32_t block, const float* edges, float* scales,
                                    int8_t* codes, void* ws, void* stream);
grace_status_t grace_u8bit_compress_bf16(const uint16_t* x, int64_t n, int32_t block, const float* edges,
                                         float* scales, int8_t* codes, void* ws, void* stream);
/* World-1 Allgather(U8bit, NoneMemory).step: scales[nblk] as above and out = 0 + d, the decode of
 * this rank's own codes summed from 0, in the gradient's type.  The codes are never stored. */
grace_status_t grace_u8bit_step_w1(const float* x, int64_t n, int32_t block, const float* edges, const float* values,
                                   float* scales, float* out, void* ws, void* stream);
grace_status_t grace_u8bit_step_w1_bf16(const uint16_t* x, int64_t n, int32_t block, const float* edges,
                                        const float* values, float* scales, uint16_t* out, void* ws, void* stream);
/* Decode + aggregate of `world` (1 to 1024) gathered payloads in one launch: rank w's codes at
 * codes + w * code_stride (code_stride >= n when world > 1), its scales at scales + w * nblk;
 * out = (((0 + d_0) + d_1) + ...) / divisor, summed in rank order in f32; no division when
 * divisor == 1. */
grace_status_t grace_u8bit_decode_aggregate(const int8_t* codes, int64_t code_stride, const float* scales,
                                            int32_t world, int64_t n, int32_t block, const float* values,
                                            float divisor, float* out, void* stream);
grace_status_t grace_u8bit_decode_aggregate_bf16(const int8_t* codes, int64_t code_stride, const float* scales,
                                                 int32_t world, int64_t n, int32_t block, const float* values,
                                                 float divisor, uint16_t* out, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* GRACE_HIP_U8BIT_H */
