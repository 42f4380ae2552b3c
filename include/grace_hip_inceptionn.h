/*
 * grace_hip_inceptionn.h — error-bounded variable-width compression (INCEPTIONN: Li et al., "A
 * Network-Centric Hardware/Algorithm Co-Design to Accelerate Distributed Training of Deep Neural
 * Networks", MICRO 2018) on float32 and bfloat16 gradients (libgrace_hip.so, gfx950;
 * grace_amd/csrc/inceptionn.hip).
 *
 * A ninth header of the same library: the rules at the top of grace_hip.h hold for every entry
 * point here (device pointers, stream-ordered, nothing allocates or synchronises, grace_status_t,
 * f32 arithmetic with every operation rounded on its own).  In addition:
 *   - a bfloat16 array travels as its 16-bit patterns, `uint16_t*`; an odd address is refused;
 *   - a bf16 gradient is widened exactly; a bf16 dense result is the f32 result rounded once to
 *     nearest even (a NaN becomes 0x7FC0);
 *   - each `_bf16` entry point differs from its f32 form only in `uint16_t*` for the gradient or the
 *     dense result: the payload is the f32 entry point's for the widened gradient;
 *   - an argument error (b outside [1, 14], n outside [0, 2^31), a null or misaligned pointer, world
 *     outside [1, 1024], a zero divisor, a stride that is no multiple of 16 or shorter than the
 *     header) returns GRACE_ERR_ARG with "<name>: ..." in grace_last_error() and touches no device;
 *     n == 0 is GRACE_OK with no launch.
 *
 * The codec.  Parameter b, 1 <= b <= 14: the bound is 2^-b.  E = 127 - b, radius = ceil(b / 2),
 * mid = E + radius, s8 = 134 - mid.  For an f32 element x let e be its biased exponent, s its sign
 * bit and a = |x|:
 *
 *   tag 3   e >= 127 (|x| >= 1, +-Inf, NaN)   the 32 bits of x                       decodes to x, bit for bit
 *   tag 2   mid <= e < 127                   u16: s << 15 | floor(a * 2^15)         +-q * 2^-15
 *   tag 1   E <= e < mid                     u8:  s << 7  | floor(a * 2^s8)         +-q * 2^-s8
 *   tag 0   e < E (zeros, denormals)         nothing                                +0.0
 *
 * Both floors are right shifts of the 24-bit significand (by 135 - e and by 16 + mid - e), so the
 * codec is integer work and every decoded value is exact in f32.  q is never 0 for tags 1 and 2,
 * q < 2^15 for tag 2 and q < 2^7 for tag 1, and |x - d| < 2^-b for every element with e < 127.  A
 * decoder takes any code: q = 0 with the sign set decodes to -0.0.
 *
 * The wire: one byte stream, 16-byte aligned, in tiles of T = 4096 elements (the last one ragged,
 * m elements); ntiles = ceil(n / T).
 *   word 0 (u32)              the payload's total length in 16-byte units, header included;
 *   words 1 .. ntiles (u32)   each tile's offset from the start of the payload, in 16-byte units;
 *                             the header is then zero-padded to 16 bytes.
 *   a tile                    (1) its tags in 16 * ceil(m / 64) bytes: element 4i + j of the tile in
 *                             bits 2j, 2j + 1 of byte i, unused tags zero; (2) its tag-3 values as
 *                             u32; (3) its tag-2 codes as u16; (4) its tag-1 codes as u8; each stream
 *                             in element order; the tile is then zero-padded to 16 bytes.
 * A tile's stream lengths are not stored: the decoder counts the tile's tags.  Tiles do not overlap
 * and with the header fill exactly [0, total).  The ORDER of the tiles inside the payload is not
 * specified and may differ between two calls on the same x (each workgroup reserves its tile's place
 * with one atomic add and waits for nobody); the bytes of each tile are specified.  The worst case
 * is grace_inceptionn_capacity_bytes(n): the header plus 16 * ceil(m / 64) + 16 * ceil(m / 4) bytes a
 * tile.  Bytes of the buffer past the total are not written.
 *
 * The vector paths (16 B of the gradient or the dense result per access) run when that array is
 * 16-byte aligned; guarded per-element accesses run otherwise and in the ragged tile, inside the
 * same kernels.  Nothing outside [0, n) of a gradient or a result is touched, and nothing outside
 * [0, capacity) of a payload written or [0, stride_bytes) of a payload read.
 */
#ifndef GRACE_HIP_INCEPTIONN_H
#define GRACE_HIP_INCEPTIONN_H

#include "grace_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The worst-case payload of n elements, in bytes (0 for an n the codec refuses, and for n == 0). */
size_t grace_inceptionn_capacity_bytes(int64_t n);

/* payload (capacity bytes, 16-byte aligned) = the wire above.  Two launches: one workgroup sets word 0
 * to the header's length and zeroes the header's padding; then one workgroup a tile, x read once. */
grace_status_t grace_inceptionn_compress(const float* x, int64_t n, int32_t b, uint8_t* payload, void* stream);
grace_status_t grace_inceptionn_compress_bf16(const uint16_t* x, int64_t n, int32_t b, uint8_t* payload,
                                              void* stream);
/* World-1 Allgather(Inceptionn, NoneMemory).step: out = d(x) elementwise in the gradient's type, with
 * no wire at all (one streaming kernel). */
grace_status_t grace_inceptionn_step_w1(const float* x, int64_t n, int32_t b, float* out, void* stream);
grace_status_t grace_inceptionn_step_w1_bf16(const uint16_t* x, int64_t n, int32_t b, uint16_t* out,
                                             void* stream);
/* Decode + aggregate of `world` (1 to 1024) gathered payloads in one launch: rank w's payload starts at
 * payloads + w * stride_bytes (16-byte aligned; stride_bytes a multiple of 16 and at least the header);
 * out = (((0 + d_0) + d_1) + ...) / divisor, summed in rank order in f32; no division when
 * divisor == 1.  A tile whose directory entry or counted extent leaves [header, stride_bytes) of its
 * rank contributes zeros for that rank and is not read. */
grace_status_t grace_inceptionn_decode_aggregate(const uint8_t* payloads, int64_t stride_bytes, int32_t world,
                                                 int64_t n, int32_t b, float divisor, float* out, void* stream);
grace_status_t grace_inceptionn_decode_aggregate_bf16(const uint8_t* payloads, int64_t stride_bytes, int32_t world,
                                                      int64_t n, int32_t b, float divisor, uint16_t* out,
                                                      void* stream);

#ifdef __cplusplus
}
#endif

#endif /* GRACE_HIP_INCEPTIONN_H */
