/*
 * grace_hip_adaq.h — adaptive quantisation (AdaQ: Dryden, Moon, Jacobs and Van Essen, "Communication
 * Quantization for Data-Parallel Training of Deep Neural Networks", MLHPC 2016) on float32 and
 * bfloat16 gradients (libgrace_hip.so, gfx950; grace_amd/csrc/adaq.hip).
 *
 * A tenth header of the same library: the rules at the top of grace_hip.h hold for every entry
 * point here (device pointers, stream-ordered, nothing allocates or synchronises, grace_status_t,
 * f32 arithmetic with every operation rounded on its own).  In addition:
 *   - a bfloat16 array travels as its 16-bit patterns, `uint16_t*`; an odd address is refused;
 *   - a bf16 gradient is widened exactly; a bf16 dense result is the f32 result rounded once to
 *     nearest even (a NaN becomes 0x7FC0);
 *   - each `_bf16` entry point differs from its f32 form only in `uint16_t*` for the gradient or the
 *     dense result: the payload is the f32 entry point's for the widened gradient;
 *   - an argument error (n outside [0, 2^31), ratio outside (0, 1] or NaN, a null or misaligned
 *     pointer, world outside [1, 1024], a zero divisor, a cap outside [0, n + 4], a stride that is no
 *     multiple of 16 or shorter than the payload, a workspace that is too small) returns
 *     GRACE_ERR_ARG with "<name>: ..." in grace_last_error() and touches no device; n == 0 is
 *     GRACE_OK with no launch.
 *
 * The codec.  x has n elements, 0 <= n < 2^31; `ratio` is a double, 0 < ratio <= 1.  All
 * classification is integer work on the bit patterns: with u the 32 bits of an element, its sign is
 * u >> 31 and its magnitude is mag = u & 0x7FFFFFFF.
 *
 *   classes    an element is positive if its sign bit is clear and mag != 0, negative if its sign bit
 *              is set and mag != 0.  +-0 belongs to neither class.  Denormals and +-Inf are ordinary
 *              members.  NaN is outside the contract: the result is unspecified, but nothing out of
 *              bounds is touched.
 *   counts     m+ and m- are the class sizes; k_s = ceil((double)m_s * ratio), one f64 product and one
 *              ceil; 0 when m_s == 0 and 1 <= k_s <= m_s otherwise.
 *   selection  in each class exactly the k_s elements of largest magnitude are selected, ties at the
 *              cut going to the lower index first: with T_s the cut magnitude, an element is selected
 *              if mag > T_s, and one with mag == T_s is selected if fewer than
 *              k_s - #{mag > T_s} same-class elements with mag == T_s precede it.
 *   means      mean_s = the f64 sum of the selected elements of the class, divided in f64 by k_s and
 *              rounded once to f32; +0.0 when k_s == 0.  The sum's order is fixed: a thread's elements
 *              in element order, a fixed tree over the workgroup, the chunks in a fixed strided order,
 *              then (ties taken) * (+-T_s) once.  The same x, n and ratio give the same bits on every
 *              call, and compress and step_w1 give the same means as each other.  The addends share
 *              a sign, so no cancellation occurs: each of at most k + 2 roundings moves the sum by at
 *              most 2^-53 of its final magnitude, and for k <= 2^29 the mean is within 1 f32 ulp of
 *              the exactly rounded value.  A mean is never -0.0 (its magnitude is at least that of
 *              the smallest selected element).
 *   decode     d_i = mean+ if element i is selected positive, mean- if selected negative, +0.0
 *              otherwise.
 *   aggregate  out = (((0 + d^0) + d^1) + ...) in f32 in rank order; one division unless the divisor
 *              is 1; a bf16 result gets one rounding to nearest even.
 *
 * The wire.  Its size is fixed by (n, ratio) and is the same for g and g.float().  C = 8192,
 * nchunks = ceil(n / C), cap = ceil((double)n * ratio) + 4; every part is 16-byte aligned.
 *
 *   header, 16 B   f32 mean+, f32 mean-, u32 count = k+ + k-, u32 cap
 *   directory      u32 ends[nchunks]: the number of entries in chunks 0 .. c; zero-padded to 16 B
 *   entries        u16 [cap]: sign << 15 | offset inside its chunk (13 bits; bits 13 and 14 zero);
 *                  zero-padded to 16 B
 *
 * The entries are one list in ascending element order, both signs merged.  Entries in [count, cap)
 * and all padding are written as zeros, so every byte of the payload is specified and two calls on
 * the same x give identical bytes.
 *
 * k+ + k- <= cap for every input.  With e = 2^-53, fl() the f64 rounding and r = ratio:
 * k_s = ceil(fl(m_s r)) < m_s r (1 + e) + 1, so k+ + k- < (m+ + m-) r (1 + e) + 2 <= n r + n r e + 2
 * < n r + 3, because n r e < 2^31 2^-53 < 1.  And cap >= fl(n r) + 4 >= n r (1 - e) + 4 > n r + 3.
 * The +4 is the room for the two ceilings and the f64 roundings.
 *
 * The vector paths (16 B of the gradient or the dense result per access) run when that array is
 * 16-byte aligned; guarded per-element accesses run otherwise and in the ragged chunk, inside the
 * same kernels.  Nothing outside [0, n) of a gradient or a result is touched, nothing outside
 * [0, grace_adaq_payload_bytes) of a payload written or [0, stride_bytes) of a payload read, and
 * nothing outside [0, ws_bytes) of the workspace.
 */
#ifndef GRACE_HIP_ADAQ_H
#define GRACE_HIP_ADAQ_H

#include "grace_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* cap of (n, ratio): the entry capacity of the wire.  0 for arguments the codec refuses and for n == 0. */
int64_t grace_adaq_capacity(int64_t n, double ratio);
/* The payload's length in bytes, a multiple of 16.  0 for arguments the codec refuses and for n == 0. */
size_t grace_adaq_payload_bytes(int64_t n, double ratio);
/* The workspace of a compress or a step on n elements, in bytes (16-byte aligned; its content between
 * calls is of no account: the codec zeroes what it counts in).  0 for an n the codec refuses. */
size_t grace_adaq_workspace_bytes(int64_t n);

/* payload (grace_adaq_payload_bytes(n, ratio) bytes, 16-byte aligned) = the wire above.  The select
 * reads x three times (bf16: twice), the count pass and the write pass once each. */
grace_status_t grace_adaq_compress(const float* x, int64_t n, double ratio, uint8_t* payload, void* ws,
                                   size_t ws_bytes, void* stream);
grace_status_t grace_adaq_compress_bf16(const uint16_t* x, int64_t n, double ratio, uint8_t* payload, void* ws,
                                        size_t ws_bytes, void* stream);
/* World-1 Allgather(Adaq, NoneMemory).step: out = d(x) elementwise in the gradient's type.  The same
 * select, count pass and scan; no entries are written. */
grace_status_t grace_adaq_step_w1(const float* x, int64_t n, double ratio, float* out, void* ws, size_t ws_bytes,
                                  void* stream);
grace_status_t grace_adaq_step_w1_bf16(const uint16_t* x, int64_t n, double ratio, uint16_t* out, void* ws,
                                       size_t ws_bytes, void* stream);
/* Decode + aggregate of `world` (1 to 1024) gathered payloads in one launch: rank w's payload starts at
 * payloads + w * stride_bytes (16-byte aligned; stride_bytes a multiple of 16 and at least the payload of
 * (n, cap)); out = (((0 + d_0) + d_1) + ...) / divisor, summed in rank order in f32; no division when
 * divisor == 1.  Every one of the n outputs is written, in one pass over the output.  A rank whose
 * header cap differs from `cap` contributes zeros and is not read further; a chunk of a rank whose
 * `ends` are not monotone or exceed min(count, cap) contributes zeros for that rank; an entry whose
 * offset lies past the end of a ragged last chunk is skipped. */
grace_status_t grace_adaq_decode_aggregate(const uint8_t* payloads, int64_t stride_bytes, int32_t world, int64_t n,
                                           int64_t cap, float divisor, float* out, void* stream);
grace_status_t grace_adaq_decode_aggregate_bf16(const uint8_t* payloads, int64_t stride_bytes, int32_t world,
                                                int64_t n, int64_t cap, float divisor, uint16_t* out, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* GRACE_HIP_ADAQ_H */
