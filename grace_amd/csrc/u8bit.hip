// 8-bit codebook quantisation with one absmax scale per block.
//
// Encode is one kernel template over <element type, rows per chunk, tensor-wide, fused>.  A wave owns
// whole chunks of R rows; a row is one 16-B load of every lane (64 * G elements: 256 f32, 512 bf16),
// and a chunk is one block of the tensor -- or two, for 256-element bf16 blocks, which are half a row
// each.  The lane keeps its R raw 16-B words in registers (16 for a 4096-element f32 block): |x| max
// in-lane, then over the lanes that share the block by DPP butterflies inside each row of 16 lanes
// and two cross-row exchanges; then the division, the search and the packed store run from the same
// registers, so x is read exactly once.  The loads of the wave's next chunk are issued before the
// search of the current one.
//
// The search is a branch-free 7-step lower bound over edges[1..127] (edges[0] only separates a count
// of 0 from a count of 1, and both are code 0).  The top three levels are seven wave-uniform
// values selected by v_cndmask; the last four levels read the table staged in LDS, the G searches of
// a lane step together so that the four rounds of LDS reads overlap.
//
// Tensor-wide (block == 0) the maximum is a pass of its own -- workgroup partials behind an arrival
// ticket, finished by the last arriver -- and the same encode kernel reads the scale from the device.
//
// A chunk that crosses n, or any chunk when an operand is not aligned for its vector access, goes
// through guarded per-element accesses in the same kernel: nothing outside [0, n) is touched.
#include "common.h"

#include "../../include/grace_hip_u8bit.h"

namespace grace {

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));

constexpr int kUBlock = 256;          // threads per workgroup: 4 waves
constexpr int kUWaves = kUBlock / kWave;
constexpr int kUGridCap = 1024;       // encode: workgroups at most (a wave loops over its chunks)
constexpr int kUDecGridCap = 4096;
constexpr int kUParts = 1024;         // tensor-wide maximum: workgroups (= partials) at most
constexpr int kUPartOff = 64;         // ws: u32 ticket at word 0, the partials from word 64 on
constexpr int kULevels = 128;
static_assert(sizeof(uint32_t) * (kUPartOff + kUParts) <= sizeof(double) * 4 * kRedBlocks,
              "the ticket and the partials fit grace_reduce_workspace_bytes");

// ------------------------------------------------------------------------------------------------
// Element access.  A lane's share of a row travels as the raw 16 B it was loaded as.
template <typename E>
struct U8;

template <>
struct U8<float> {
  static constexpr int G = 4;
  static bool addressable(const void* p) { return al4(p); }
  static __device__ __forceinline__ void unpack(u32x4 t, float (&v)[4]) {
    v[0] = u2f(t[0]); v[1] = u2f(t[1]); v[2] = u2f(t[2]); v[3] = u2f(t[3]);
  }
  static __device__ __forceinline__ u32x4 gather(const float* p, int64_t e, int64_t n) {
    u32x4 t;
#pragma unroll
    for (int j = 0; j < 4; ++j) t[j] = e + j < n ? f2u(p[e + j]) : 0u;
    return t;
  }
  static __device__ __forceinline__ u32x4 pack(const float (&d)[4]) {
    u32x4 t;
#pragma unroll
    for (int j = 0; j < 4; ++j) t[j] = f2u(d[j]);
    return t;
  }
  static __device__ __forceinline__ void st(float* p, int64_t i, float v) { p[i] = v; }
};

template <>
struct U8<uint16_t> {
  static constexpr int G = 8;
  static bool addressable(const void* p) { return al2(p); }
  static __device__ __forceinline__ void unpack(u32x4 t, float (&v)[8]) {
#pragma unroll
    for (int k = 0; k < 4; ++k) { v[2 * k] = u2f(t[k] << 16); v[2 * k + 1] = u2f(t[k] & 0xFFFF0000u); }
  }
  static __device__ __forceinline__ u32x4 gather(const uint16_t* p, int64_t e, int64_t n) {
    u32x4 t;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const uint32_t lo = e + 2 * k < n ? (uint32_t)p[e + 2 * k] : 0u;
      const uint32_t hi = e + 2 * k + 1 < n ? (uint32_t)p[e + 2 * k + 1] : 0u;
      t[k] = lo | (hi << 16);
    }
    return t;
  }
  static __device__ __forceinline__ u32x4 pack(const float (&d)[8]) {
    u32x4 t;
#pragma unroll
    for (int k = 0; k < 4; ++k) t[k] = pack_bf16x2(d[2 * k], d[2 * k + 1]);
    return t;
  }
  static __device__ __forceinline__ void st(uint16_t* p, int64_t i, float v) { p[i] = f32_to_bf16(v); }
};

template <typename E>
__device__ __forceinline__ u32x4 load_raw(const E* x, int64_t e, int64_t n, bool fast) {
  if (fast) return __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(x + e));
  return U8<E>::gather(x, e, n);
}

template <typename E>
__device__ __forceinline__ void store_dense(E* o, int64_t e, int64_t n, bool fast, const float (&d)[U8<E>::G]) {
  if (fast) {
    __builtin_nontemporal_store(U8<E>::pack(d), reinterpret_cast<u32x4*>(o + e));
  } else {
#pragma unroll
    for (int j = 0; j < U8<E>::G; ++j)
      if (e + j < n) U8<E>::st(o, e + j, d[j]);
  }
}

__device__ __forceinline__ uint32_t pack_i8x4(const int32_t* c) {
  return (uint32_t)(c[0] & 0xFF) | ((uint32_t)(c[1] & 0xFF) << 8) | ((uint32_t)(c[2] & 0xFF) << 16) |
         ((uint32_t)c[3] << 24);
}

template <int G>
__device__ __forceinline__ void store_codes(int8_t* c, int64_t e, int64_t n, bool fast, const int32_t (&b)[G]) {
  if (fast) {
    if constexpr (G == 4) {
      __builtin_nontemporal_store(pack_i8x4(b), reinterpret_cast<uint32_t*>(c + e));
    } else {
      u32x2 t;
      t[0] = pack_i8x4(b); t[1] = pack_i8x4(b + 4);
      __builtin_nontemporal_store(t, reinterpret_cast<u32x2*>(c + e));
    }
  } else {
#pragma unroll
    for (int j = 0; j < G; ++j)
      if (e + j < n) c[e + j] = (int8_t)b[j];
  }
}

template <int G>
__device__ __forceinline__ void load_codes(const int8_t* c, int64_t e, int64_t n, bool fast, int32_t (&b)[G]) {
  if (fast) {
    uint32_t w[G / 4];
    if constexpr (G == 4) {
      w[0] = *reinterpret_cast<const uint32_t*>(c + e);
    } else {
      const u32x2 t = *reinterpret_cast<const u32x2*>(c + e);
      w[0] = t[0]; w[1] = t[1];
    }
#pragma unroll
    for (int j = 0; j < G; ++j) b[j] = (int32_t)(int8_t)(w[j >> 2] >> (8 * (j & 3)));
  } else {
#pragma unroll
    for (int j = 0; j < G; ++j) b[j] = e + j < n ? (int32_t)c[e + j] : 0;
  }
}

// Ordering key of |x| with NaN ignored: NaN counts as 0, the identity of the maximum.
__device__ __forceinline__ uint32_t max_key(float x) {
  const uint32_t k = abs_key(x);
  return k > 0x7F800000u ? 0u : k;
}

// Maximum over the lanes that share a block: inside each row of 16 lanes by row16_max (common.h),
// then over the rows: xor 16 joins the rows of a half-wave, xor 32 the halves (skipped when each half
// has its own block).
__device__ __forceinline__ uint32_t block_lanes_max(uint32_t m, bool halves) {
  m = row16_max(m);
  m = max(m, (uint32_t)__shfl_xor((int)m, 16, 64));
  if (!halves) m = max(m, (uint32_t)__shfl_xor((int)m, 32, 64));
  return m;
}

// The seven edges of the search's top three levels, the same in every lane.
struct TopEdges { float e64, e32, e96, e16, e48, e80, e112; };

// i = #{j in 1..127 : edges[j] <= y} for G values at once.  A NaN y compares false everywhere: 0.
template <int G>
__device__ __forceinline__ void search(const float (&y)[G], const TopEdges& t, const float* __restrict__ sh_e,
                                       int32_t (&pos)[G]) {
#pragma unroll
  for (int j = 0; j < G; ++j) pos[j] = t.e64 <= y[j] ? 64 : 0;
#pragma unroll
  for (int j = 0; j < G; ++j) pos[j] += (pos[j] ? t.e96 : t.e32) <= y[j] ? 32 : 0;
#pragma unroll
  for (int j = 0; j < G; ++j) {
    const float lo = (pos[j] & 32) ? t.e48 : t.e16, hi = (pos[j] & 32) ? t.e112 : t.e80;
    pos[j] += ((pos[j] & 64) ? hi : lo) <= y[j] ? 16 : 0;
  }
#pragma unroll
  for (int s = 8; s > 0; s >>= 1) {
    float e[G];
#pragma unroll
    for (int j = 0; j < G; ++j) e[j] = sh_e[pos[j] + s];
#pragma unroll
    for (int j = 0; j < G; ++j) pos[j] += e[j] <= y[j] ? s : 0;
  }
}

// ------------------------------------------------------------------------------------------------
// tensor-wide maximum: partials per workgroup, the last arriver (told by its ticket) finishes
__device__ __forceinline__ uint32_t workgroup_max(uint32_t m, uint32_t* sh) {
  m = block_lanes_max(m, false);
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = m;
  __syncthreads();
  uint32_t t = 0;
#pragma unroll
  for (int w = 0; w < kUWaves; ++w) t = max(t, sh[w]);
  return t;
}

template <typename E>
__global__ __launch_bounds__(kUBlock) void u8_absmax_e(const E* __restrict__ x, int64_t n, uint32_t* __restrict__ ws,
                                                       float* __restrict__ scales, int aligned) {
  constexpr int G = U8<E>::G;
  __shared__ uint32_t sh[kUWaves], sh2[kUWaves], s_last;
  const int64_t ng = (n + G - 1) / G;
  uint32_t m = 0;
#pragma unroll 4
  for (int64_t g = (int64_t)blockIdx.x * kUBlock + threadIdx.x; g < ng; g += (int64_t)gridDim.x * kUBlock) {
    const int64_t e = g * G;
    float v[G];
    U8<E>::unpack(load_raw<E>(x, e, n, aligned && e + G <= n), v);
#pragma unroll
    for (int j = 0; j < G; ++j) m = max(m, max_key(v[j]));
  }
  m = workgroup_max(m, sh);
  // arrival (DESIGN §4 memory-model table, row 1): lane 0 alone stores the partial write-through,
  // waits for it and adds to the ticket, so it signals only for its own store
  if (threadIdx.x == 0) {
    __hip_atomic_store(ws + kUPartOff + blockIdx.x, m, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    s_last = atomicAdd(ws, 1u) == gridDim.x - 1 ? 1u : 0u;
  }
  __syncthreads();
  if (!s_last) return;
  // the last arriver: acquire after the ticket, then sc1 loads of every partial
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
  uint32_t t = 0;
  for (int b = threadIdx.x; b < (int)gridDim.x; b += kUBlock)
    t = max(t, __hip_atomic_load(ws + kUPartOff + b, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
  t = workgroup_max(t, sh2);
  if (threadIdx.x == 0) {
    scales[0] = u2f(t);
    __hip_atomic_store(ws, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // the next call's ticket
  }
}

// ------------------------------------------------------------------------------------------------
// encode / fused world-1 step
template <typename E, int R, bool TENSOR, bool FUSED>
__global__ __launch_bounds__(kUBlock) void u8_encode_e(const E* __restrict__ x, int64_t n, int halves,
                                                       const float* __restrict__ edges,
                                                       const float* __restrict__ values, float* __restrict__ scales,
                                                       int64_t nblk, int8_t* __restrict__ codes, E* __restrict__ out,
                                                       int aligned) {
  constexpr int G = U8<E>::G;
  constexpr int kRow = kWave * G;
  constexpr int64_t C = (int64_t)R * kRow;
  __shared__ float sh_e[kULevels];
  __shared__ float sh_v[FUSED ? kULevels : 1];
  if (threadIdx.x < kULevels) {
    sh_e[threadIdx.x] = edges[threadIdx.x];
    if constexpr (FUSED) sh_v[threadIdx.x] = values[threadIdx.x];
  }
  const TopEdges top{edges[64], edges[32], edges[96], edges[16], edges[48], edges[80], edges[112]};
  float a_tensor = 0.f;
  if constexpr (TENSOR) a_tensor = scales[0];
  __syncthreads();

  const int lane = threadIdx.x & 63;
  const int64_t nchunks = (n + C - 1) / C;
  const int64_t nwaves = (int64_t)gridDim.x * kUWaves;
  int64_t c = (int64_t)blockIdx.x * kUWaves + (threadIdx.x >> 6);
  u32x4 cur[R], nxt[R];
#pragma unroll
  for (int r = 0; r < R; ++r) { cur[r] = (u32x4)(0u); nxt[r] = (u32x4)(0u); }
  if (c < nchunks) {
    const bool fast = aligned && (c + 1) * C <= n;
#pragma unroll
    for (int r = 0; r < R; ++r) cur[r] = load_raw<E>(x, c * C + r * kRow + lane * G, n, fast);
  }
  for (; c < nchunks; c += nwaves) {
    const int64_t c2 = c + nwaves;
    if (c2 < nchunks) {   // the next chunk's loads fly over this chunk's reduction, search and stores
      const bool fast2 = aligned && (c2 + 1) * C <= n;
#pragma unroll
      for (int r = 0; r < R; ++r) nxt[r] = load_raw<E>(x, c2 * C + r * kRow + lane * G, n, fast2);
    }
    const bool fast = aligned && (c + 1) * C <= n;
    float a = a_tensor;
    if constexpr (!TENSOR) {
      uint32_t m = 0;
#pragma unroll
      for (int r = 0; r < R; ++r) {
        float v[G];
        U8<E>::unpack(cur[r], v);
#pragma unroll
        for (int j = 0; j < G; ++j) m = max(m, max_key(v[j]));
      }
      a = u2f(block_lanes_max(m, halves != 0));
      const int64_t b = halves ? 2 * c + (lane >> 5) : c;
      if ((lane & (halves ? 31 : 63)) == 0 && b < nblk) scales[b] = a;
    }
#pragma unroll
    for (int r = 0; r < R; ++r) {
      const int64_t e = c * C + r * kRow + lane * G;
      float v[G], y[G];
      int32_t pos[G];
      U8<E>::unpack(cur[r], v);
#pragma unroll
      for (int j = 0; j < G; ++j) y[j] = fabsf(v[j]) / a;
      search<G>(y, top, sh_e, pos);
      if constexpr (FUSED) {
        float d[G];
#pragma unroll
        for (int j = 0; j < G; ++j) {
          const float mag = sh_v[pos[j]] * a;
          d[j] = 0.f + (pos[j] == 0 ? 0.f : (v[j] < 0.f ? -mag : mag));
        }
        store_dense<E>(out, e, n, fast, d);
      } else {
#pragma unroll
        for (int j = 0; j < G; ++j) pos[j] = v[j] < 0.f ? -pos[j] : pos[j];
        store_codes<G>(codes, e, n, fast, pos);
      }
    }
#pragma unroll
    for (int r = 0; r < R; ++r) cur[r] = nxt[r];
  }
}

// ------------------------------------------------------------------------------------------------
// decode + aggregate: W rank-major payloads, summed in rank order, one division, one rounding
template <typename O>
__global__ __launch_bounds__(kUBlock) void u8_decode_e(const int8_t* __restrict__ codes, int64_t stride,
                                                       const float* __restrict__ scales, int world, int64_t n,
                                                       int shift, int64_t nblk, const float* __restrict__ values,
                                                       float divisor, O* __restrict__ out, int aligned) {
  constexpr int G = U8<O>::G;
  __shared__ float sh_v[kULevels];
  if (threadIdx.x < kULevels) sh_v[threadIdx.x] = values[threadIdx.x];
  __syncthreads();
  const int64_t ng = (n + G - 1) / G;
  for (int64_t g = (int64_t)blockIdx.x * kUBlock + threadIdx.x; g < ng; g += (int64_t)gridDim.x * kUBlock) {
    const int64_t e = g * G;
    const bool fast = aligned && e + G <= n;
    const int64_t b = shift < 0 ? 0 : e >> shift;   // G divides the block: one scale per group and rank
    float acc[G];
#pragma unroll
    for (int j = 0; j < G; ++j) acc[j] = 0.f;
    for (int w = 0; w < world; ++w) {
      const float a = scales[w * nblk + b];
      int32_t cd[G];
      load_codes<G>(codes + w * stride, e, n, fast, cd);
#pragma unroll
      for (int j = 0; j < G; ++j) {
        const float mag = sh_v[(cd[j] < 0 ? -cd[j] : cd[j]) & (kULevels - 1)] * a;
        acc[j] = acc[j] + (cd[j] == 0 ? 0.f : (cd[j] < 0 ? -mag : mag));
      }
    }
#pragma unroll
    for (int j = 0; j < G; ++j) acc[j] = divisor == 1.0f ? acc[j] : acc[j] / divisor;
    store_dense<O>(out, e, n, fast, acc);
  }
}

// ------------------------------------------------------------------------------------------------
// host side: one typed launcher per f32 / bf16 pair
static inline bool block_ok(int32_t block) {
  return block == 0 || (block >= 256 && block <= 4096 && (block & (block - 1)) == 0);
}

template <typename E, int R, bool FUSED>
static void launch_rows(unsigned grid, hipStream_t st, const E* x, int64_t n, int halves, const float* edges,
                        const float* values, float* scales, int64_t nblk, int8_t* codes, E* out, int al) {
  u8_encode_e<E, R, false, FUSED><<<grid, kUBlock, 0, st>>>(x, n, halves, edges, values, scales, nblk, codes, out, al);
}

template <typename E, bool FUSED>
static grace_status_t u8_encode(const char* name, const char* bad, const E* x, int64_t n, int32_t block,
                                const float* edges, const float* values, float* scales, int8_t* codes, E* out,
                                void* ws, void* stream) {
  GRACE_REQUIRE(x && edges && scales && (FUSED ? values && out : codes != nullptr) && n >= 0 && block_ok(block) &&
                    (block != 0 || (ws && al4(ws))) &&
                    U8<E>::addressable(x) && (!FUSED || U8<E>::addressable(out)) && al4(edges) && al4(values) &&
                    al4(scales),
                bad);
  if (n == 0) return GRACE_OK;
  constexpr int G = U8<E>::G;
  constexpr int kRow = kWave * G;
  const hipStream_t st = as_stream(stream);
  const int al = al16(x) && (FUSED ? al16(out) : (G == 8 ? al8(codes) : al4(codes)));
  if (block == 0) {
    const unsigned parts = stream_grid((n + G - 1) / G, kUBlock, kUParts);
    u8_absmax_e<E><<<parts, kUBlock, 0, st>>>(x, n, reinterpret_cast<uint32_t*>(ws), scales, al16(x) ? 1 : 0);
    GRACE_CHECK_LAUNCH(name);
    const unsigned grid = stream_grid((n + kRow - 1) / kRow, kUWaves, kUGridCap);
    u8_encode_e<E, 1, true, FUSED><<<grid, kUBlock, 0, st>>>(x, n, 0, edges, values, scales, 1, codes, out, al);
    GRACE_CHECK_LAUNCH(name);
    return GRACE_OK;
  }
  const int halves = block < kRow ? 1 : 0;          // 256-element bf16 blocks: two to a row
  const int rows = halves ? 1 : block / kRow;
  const int64_t chunk = (int64_t)rows * kRow;
  const int64_t nblk = (n + block - 1) / block;
  const unsigned grid = stream_grid((n + chunk - 1) / chunk, kUWaves, kUGridCap);
  switch (rows) {
    case 1: launch_rows<E, 1, FUSED>(grid, st, x, n, halves, edges, values, scales, nblk, codes, out, al); break;
    case 2: launch_rows<E, 2, FUSED>(grid, st, x, n, halves, edges, values, scales, nblk, codes, out, al); break;
    case 4: launch_rows<E, 4, FUSED>(grid, st, x, n, halves, edges, values, scales, nblk, codes, out, al); break;
    case 8: launch_rows<E, 8, FUSED>(grid, st, x, n, halves, edges, values, scales, nblk, codes, out, al); break;
    default: launch_rows<E, 16, FUSED>(grid, st, x, n, halves, edges, values, scales, nblk, codes, out, al); break;
  }
  GRACE_CHECK_LAUNCH(name);
  return GRACE_OK;
}

template <typename O>
static grace_status_t u8_decode(const char* name, const char* bad, const int8_t* codes, int64_t stride,
                                const float* scales, int32_t world, int64_t n, int32_t block, const float* values,
                                float divisor, O* out, void* stream) {
  GRACE_REQUIRE(codes && scales && values && out && world >= 1 && world <= 1024 && n >= 0 && block_ok(block) &&
                    divisor != 0.0f && (world == 1 || stride >= n) && al4(scales) && al4(values) &&
                    U8<O>::addressable(out),
                bad);
  if (n == 0) return GRACE_OK;
  constexpr int G = U8<O>::G;
  const int shift = block ? __builtin_ctz((unsigned)block) : -1;
  const int64_t nblk = block ? (n + block - 1) / block : 1;
  const int al = (G == 8 ? al8(codes) : al4(codes)) && (world == 1 || stride % G == 0) && al16(out);
  u8_decode_e<O><<<stream_grid((n + G - 1) / G, kUBlock, kUDecGridCap), kUBlock, 0, as_stream(stream)>>>(
      codes, stride, scales, world, n, shift, nblk, values, divisor, out, al);
  GRACE_CHECK_LAUNCH(name);
  return GRACE_OK;
}

}  // namespace grace

using namespace grace;

extern "C" {

grace_status_t grace_u8bit_compress(const float* x, int64_t n, int32_t block, const float* edges, float* scales,
                                    int8_t* codes, void* ws, void* stream) {
  return u8_encode<float, false>("grace_u8bit_compress", "grace_u8bit_compress: bad arguments", x, n, block, edges,
                                 nullptr, scales, codes, nullptr, ws, stream);
}

grace_status_t grace_u8bit_compress_bf16(const uint16_t* x, int64_t n, int32_t block, const float* edges,
                                         float* scales, int8_t* codes, void* ws, void* stream) {
  return u8_encode<uint16_t, false>("grace_u8bit_compress_bf16", "grace_u8bit_compress_bf16: bad arguments", x, n,
                                    block, edges, nullptr, scales, codes, nullptr, ws, stream);
}

grace_status_t grace_u8bit_step_w1(const float* x, int64_t n, int32_t block, const float* edges, const float* values,
                                   float* scales, float* out, void* ws, void* stream) {
  return u8_encode<float, true>("grace_u8bit_step_w1", "grace_u8bit_step_w1: bad arguments", x, n, block, edges,
                                values, scales, nullptr, out, ws, stream);
}

grace_status_t grace_u8bit_step_w1_bf16(const uint16_t* x, int64_t n, int32_t block, const float* edges,
                                        const float* values, float* scales, uint16_t* out, void* ws, void* stream) {
  return u8_encode<uint16_t, true>("grace_u8bit_step_w1_bf16", "grace_u8bit_step_w1_bf16: bad arguments", x, n, block,
                                   edges, values, scales, nullptr, out, ws, stream);
}

grace_status_t grace_u8bit_decode_aggregate(const int8_t* codes, int64_t code_stride, const float* scales,
                                            int32_t world, int64_t n, int32_t block, const float* values,
                                            float divisor, float* out, void* stream) {
  return u8_decode<float>("grace_u8bit_decode_aggregate", "grace_u8bit_decode_aggregate: bad arguments", codes,
                          code_stride, scales, world, n, block, values, divisor, out, stream);
}

grace_status_t grace_u8bit_decode_aggregate_bf16(const int8_t* codes, int64_t code_stride, const float* scales,
                                                 int32_t world, int64_t n, int32_t block, const float* values,
                                                 float divisor, uint16_t* out, void* stream) {
  return u8_decode<uint16_t>("grace_u8bit_decode_aggregate_bf16", "grace_u8bit_decode_aggregate_bf16: bad arguments",
                             codes, code_stride, scales, world, n, block, values, divisor, out, stream);
}

}  // extern "C"
