// Error-bounded variable-width compression (INCEPTIONN; include/grace_hip_inceptionn.h):
// a dense stream of 0 / 8 / 16 / 32-bit values behind 2-bit tags, packed tile by tile and decoded in
// parallel through a tile directory.
//
// Work split, encode and decode alike: one workgroup of 256 threads per tile of 4096 elements, 16
// consecutive elements per thread, so a thread's 16 tags are one 32-bit word of the tile's tag
// region and its codes are one run of each stream.
//
//   encode   a thread classifies its 16 elements in registers and counts its tags with three
//            popcounts; a workgroup scan (wave scan of two packed words, one LDS step across the
//            four waves) gives its byte position in each of the three streams; thread 0 reserves the
//            tile's place with one atomic add on word 0 of the payload and writes the directory
//            entry while the workgroup assembles the tile in LDS (17 KB at most); the tile leaves LDS
//            in 16-byte stores.  x is read once.  No workgroup waits for another, which is why the
//            order of the tiles in the payload is free.
//   decode   for each rank in rank order: the directory entry, the thread's tag word, the same
//            counts and scan, the tile's value bytes into LDS with 16-byte loads, then every thread
//            walks its 16 tags and its three runs in LDS and adds into 16 registers.  A tile whose
//            entry or counted extent leaves the rank's bytes is skipped, so a payload that was not
//            written by the encoder cannot make the kernel read outside it (or outside LDS: the
//            positions come from the same counts as the extent).
//   step     world 1 needs no wire: d(x) is x with the significand bits below the code's last bit
//            cleared, one streaming kernel.
//
// Operands off their 16-byte grid and the ragged tile go through guarded per-element accesses in the
// same kernels.
#include "common.h"

#include "../../include/grace_hip_inceptionn.h"

namespace grace {

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

constexpr int kIncBlock = 256;
constexpr int kIncWaves = kIncBlock / kWave;
constexpr int kIncPer = 16;                        // elements a thread: its tags are one u32
constexpr int kIncTile = kIncBlock * kIncPer;      // 4096
constexpr int kIncTagBytes = kIncTile / 4;         // 1024
constexpr int kIncValBytes = kIncTile * 4;         // every element tag 3
constexpr int kIncStepGridCap = 2048;              // the world-1 step: one sweep = 2^21 f32 / 2^22 bf16 elements
static_assert(kIncPer * 2 == 32 && kIncValBytes % 16 == 0, "a thread's tags fill one word");

// the gradient's elements as f32 bit patterns; the dense result from f32
template <typename E>
struct IncE;
template <>
struct IncE<float> {
  static constexpr int G = 4;                      // elements in 16 B
  static bool addressable(const void* p) { return al4(p); }
  static __device__ __forceinline__ uint32_t ld(const float* p, int64_t i) { return f2u(p[i]); }
  static __device__ __forceinline__ void st(float* p, int64_t i, float v) { p[i] = v; }
  static __device__ __forceinline__ void unpack(u32x4 v, uint32_t* u) {
#pragma unroll
    for (int j = 0; j < 4; ++j) u[j] = v[j];
  }
  static __device__ __forceinline__ u32x4 pack(const float* d) {
    u32x4 v;
#pragma unroll
    for (int j = 0; j < 4; ++j) v[j] = f2u(d[j]);
    return v;
  }
};
template <>
struct IncE<uint16_t> {
  static constexpr int G = 8;
  static bool addressable(const void* p) { return al2(p); }
  static __device__ __forceinline__ uint32_t ld(const uint16_t* p, int64_t i) { return (uint32_t)p[i] << 16; }
  static __device__ __forceinline__ void st(uint16_t* p, int64_t i, float v) { p[i] = f32_to_bf16(v); }
  static __device__ __forceinline__ void unpack(u32x4 v, uint32_t* u) {
#pragma unroll
    for (int j = 0; j < 4; ++j) { u[2 * j] = v[j] << 16; u[2 * j + 1] = v[j] & 0xFFFF0000u; }
  }
  static __device__ __forceinline__ u32x4 pack(const float* d) {
    u32x4 v;
#pragma unroll
    for (int j = 0; j < 4; ++j) v[j] = pack_bf16x2(d[2 * j], d[2 * j + 1]);
    return v;
  }
};

// u[j] = the bits of x[e + j], N elements; 0 (tag 0) where e + j >= n
template <typename E, int N>
__device__ __forceinline__ void load_bits(const E* x, int64_t e, int64_t n, bool fast, uint32_t (&u)[N]) {
  constexpr int G = IncE<E>::G;
  if (fast) {
#pragma unroll
    for (int g = 0; g < N / G; ++g) IncE<E>::unpack(reinterpret_cast<const u32x4*>(x + e)[g], u + g * G);
  } else {
#pragma unroll
    for (int j = 0; j < N; ++j) u[j] = e + j < n ? IncE<E>::ld(x, e + j) : 0u;
  }
}

template <typename O, int N>
__device__ __forceinline__ void store_vals(O* o, int64_t e, int64_t n, bool fast, const float (&d)[N]) {
  constexpr int G = IncE<O>::G;
  if (fast) {
#pragma unroll
    for (int g = 0; g < N / G; ++g)
      __builtin_nontemporal_store(IncE<O>::pack(d + g * G), reinterpret_cast<u32x4*>(o + e) + g);
  } else {
#pragma unroll
    for (int j = 0; j < N; ++j)
      if (e + j < n) IncE<O>::st(o, e + j, d[j]);
  }
}

// ------------------------------------------------------------------------------------------------
// the codec on one element: `lo` = E and `mid` are the exponent thresholds of tags 1 and 2
__device__ __forceinline__ uint32_t inc_tag(uint32_t u, uint32_t lo, uint32_t mid) {
  const uint32_t ex = (u >> 23) & 255u;
  return (ex >= lo ? 1u : 0u) + (ex >= mid ? 1u : 0u) + (ex >= 127u ? 1u : 0u);
}
// floor(|x| * 2^15) and floor(|x| * 2^s8) as shifts of the 24-bit significand, under the sign
__device__ __forceinline__ uint32_t inc_code16(uint32_t u) {
  return ((u >> 31) << 15) | (((u & 0x7FFFFFu) | 0x800000u) >> (135u - ((u >> 23) & 255u)));
}
__device__ __forceinline__ uint32_t inc_code8(uint32_t u, uint32_t mid) {
  return ((u >> 31) << 7) | (((u & 0x7FFFFFu) | 0x800000u) >> (16u + mid - ((u >> 23) & 255u)));
}
__device__ __forceinline__ float inc_dec16(uint32_t c) {
  return u2f(f2u((float)(c & 0x7FFFu) * 0x1p-15f) | ((c >> 15) << 31));
}
__device__ __forceinline__ float inc_dec8(uint32_t c, float scale) {
  return u2f(f2u((float)(c & 0x7Fu) * scale) | ((c >> 7) << 31));
}
// d(x) without the codes: the floor clears the significand bits under the code's last bit
__device__ __forceinline__ uint32_t inc_round_trip(uint32_t u, uint32_t lo, uint32_t mid) {
  const uint32_t ex = (u >> 23) & 255u;
  if (ex >= 127u) return u;
  if (ex >= mid) return u & (0xFFFFFFFFu << (135u - ex));
  if (ex >= lo) return u & (0xFFFFFFFFu << (16u + mid - ex));
  return 0u;
}

// the tags of 16 elements as counts: c3 | c2 << 16 (a tile's totals are at most 4096 each), and c1
__device__ __forceinline__ void inc_counts(uint32_t tags, uint32_t& c32, uint32_t& c1) {
  const uint32_t lo = tags & 0x55555555u, hi = (tags >> 1) & 0x55555555u;
  c32 = (uint32_t)__popc(lo & hi) | ((uint32_t)__popc(hi & ~lo) << 16);
  c1 = (uint32_t)__popc(lo & ~hi);
}

// Workgroup exclusive scan of two words a thread: a wave scan, then one LDS step across the four
// waves; (ta, tb) are the totals.  One barrier; the caller keeps another between two scans.
__device__ __forceinline__ void inc_scan(uint32_t a, uint32_t b, uint32_t* s_a, uint32_t* s_b, uint32_t& ea,
                                         uint32_t& eb, uint32_t& ta, uint32_t& tb) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  uint32_t ia = a, ib = b;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const uint32_t ua = __shfl_up(ia, o, 64), ub = __shfl_up(ib, o, 64);
    if (lane >= o) { ia += ua; ib += ub; }
  }
  if (lane == 63) { s_a[w] = ia; s_b[w] = ib; }
  __syncthreads();
  ea = ia - a; eb = ib - b; ta = 0; tb = 0;
#pragma unroll
  for (int i = 0; i < kIncWaves; ++i) {
    const uint32_t va = s_a[i], vb = s_b[i];
    if (i < w) { ea += va; eb += vb; }
    ta += va; tb += vb;
  }
}

static inline int64_t inc_tiles(int64_t n) { return (n + kIncTile - 1) / kIncTile; }
static inline int64_t inc_header_units(int64_t n) { return (inc_tiles(n) + 1 + 3) / 4; }

// ------------------------------------------------------------------------------------------------
// encode
// One workgroup, first: word 0 = the header's length, the header's padding = 0.
__global__ __launch_bounds__(kWave) void inc_init(uint32_t* __restrict__ payload, uint32_t ntiles) {
  const uint32_t t = threadIdx.x, units = (ntiles + 4) / 4;
  if (t == 0) payload[0] = units;
  else if (t < 4 && ntiles + t < 4 * units) payload[ntiles + t] = 0u;
}

template <typename E>
__global__ __launch_bounds__(kIncBlock) void inc_encode_e(const E* __restrict__ x, int64_t n, uint32_t lo, uint32_t mid,
                                                          uint8_t* __restrict__ payload, int aligned) {
  __shared__ u32x4 sh_tile[(kIncTagBytes + kIncValBytes) / 16];
  __shared__ uint32_t s_a[kIncWaves], s_b[kIncWaves], s_off;
  const uint32_t t = threadIdx.x;
  const int64_t tile = blockIdx.x, e0 = tile * kIncTile + t * kIncPer;
  const uint32_t m = (uint32_t)min((int64_t)kIncTile, n - tile * kIncTile);
  uint32_t u[kIncPer];
  load_bits<E>(x, e0, n, aligned && e0 + kIncPer <= n, u);
  uint32_t tags = 0;
#pragma unroll
  for (int k = 0; k < kIncPer; ++k) tags |= inc_tag(u[k], lo, mid) << (2 * k);
  uint32_t c32, c1, e32, e1, t32, t1;
  inc_counts(tags, c32, c1);
  inc_scan(c32, c1, s_a, s_b, e32, e1, t32, t1);

  const uint32_t tagbytes = 16u * ((m + 63u) / 64u);
  const uint32_t base2 = tagbytes + 4u * (t32 & 0xFFFFu), base1 = base2 + 2u * (t32 >> 16);
  const uint32_t end = base1 + t1, units = (end + 15u) >> 4;
  uint32_t* words = reinterpret_cast<uint32_t*>(payload);
  uint32_t off = 0;
  if (t == 0) off = atomicAdd(words, units);       // in flight while the tile is assembled
  uint8_t* sh8 = reinterpret_cast<uint8_t*>(sh_tile);
  if (4u * t < tagbytes) reinterpret_cast<uint32_t*>(sh_tile)[t] = tags;   // past m: zero tags
  uint32_t o3 = tagbytes + 4u * (e32 & 0xFFFFu), o2 = base2 + 2u * (e32 >> 16), o1 = base1 + e1;
#pragma unroll
  for (int k = 0; k < kIncPer; ++k) {
    const uint32_t tag = (tags >> (2 * k)) & 3u;
    if (tag == 3u) {
      *reinterpret_cast<uint32_t*>(sh8 + o3) = u[k];
      o3 += 4u;
    } else if (tag == 2u) {
      *reinterpret_cast<uint16_t*>(sh8 + o2) = (uint16_t)inc_code16(u[k]);
      o2 += 2u;
    } else if (tag == 1u) {
      sh8[o1] = (uint8_t)inc_code8(u[k], mid);
      o1 += 1u;
    }
  }
  if (t < 16u * units - end) sh8[end + t] = 0;     // the tile's padding
  if (t == 0) {
    words[1 + tile] = off;
    s_off = off;
  }
  __syncthreads();
  u32x4* dst = reinterpret_cast<u32x4*>(payload + (size_t)s_off * 16u);
  for (uint32_t i = t; i < units; i += kIncBlock) dst[i] = sh_tile[i];
}

// ------------------------------------------------------------------------------------------------
// decode + aggregate
template <typename O>
__global__ __launch_bounds__(kIncBlock) void inc_decode_e(const uint8_t* __restrict__ payloads, int64_t stride, int world,
                                                          int64_t n, uint32_t hdr_units, float scale8, float divisor,
                                                          O* __restrict__ out, int aligned) {
  __shared__ u32x4 sh_v[kIncValBytes / 16];
  __shared__ uint32_t s_a[kIncWaves], s_b[kIncWaves];
  const uint32_t t = threadIdx.x;
  const int64_t tile = blockIdx.x, e0 = tile * kIncTile + t * kIncPer;
  const uint32_t m = (uint32_t)min((int64_t)kIncTile, n - tile * kIncTile);
  const uint32_t tagbytes = 16u * ((m + 63u) / 64u);
  const uint8_t* sh8 = reinterpret_cast<const uint8_t*>(sh_v);
  float acc[kIncPer];
#pragma unroll
  for (int k = 0; k < kIncPer; ++k) acc[k] = 0.f;

  for (int w = 0; w < world; ++w) {
    const uint8_t* p = payloads + (int64_t)w * stride;
    const int64_t byte0 = 16 * (int64_t)reinterpret_cast<const uint32_t*>(p)[1 + tile];   // inside the header: the host checked
    bool ok = byte0 >= 16 * (int64_t)hdr_units && byte0 + tagbytes <= stride;
    const uint32_t tags = ok && 4u * t < tagbytes ? reinterpret_cast<const uint32_t*>(p + byte0)[t] : 0u;
    uint32_t c32, c1, e32, e1, t32, t1;
    inc_counts(tags, c32, c1);
    inc_scan(c32, c1, s_a, s_b, e32, e1, t32, t1);
    const uint32_t base2 = 4u * (t32 & 0xFFFFu), base1 = base2 + 2u * (t32 >> 16);
    const uint32_t nv = (base1 + t1 + 15u) >> 4;   // at most 16 B a thread: kIncValBytes / 16 in all
    ok = ok && byte0 + tagbytes + 16 * (int64_t)nv <= stride;
    if (ok) {
      const u32x4* src = reinterpret_cast<const u32x4*>(p + byte0 + tagbytes);
      for (uint32_t i = t; i < nv; i += kIncBlock) sh_v[i] = src[i];
    }
    __syncthreads();
    if (ok) {
      uint32_t o3 = 4u * (e32 & 0xFFFFu), o2 = base2 + 2u * (e32 >> 16), o1 = base1 + e1;
#pragma unroll
      for (int k = 0; k < kIncPer; ++k) {
        const uint32_t tag = (tags >> (2 * k)) & 3u;
        float d = 0.f;
        if (tag == 3u) {
          d = u2f(*reinterpret_cast<const uint32_t*>(sh8 + o3));
          o3 += 4u;
        } else if (tag == 2u) {
          d = inc_dec16(*reinterpret_cast<const uint16_t*>(sh8 + o2));
          o2 += 2u;
        } else if (tag == 1u) {
          d = inc_dec8(sh8[o1], scale8);
          o1 += 1u;
        }
        acc[k] = acc[k] + d;
      }
    }
    __syncthreads();                               // the next rank overwrites sh_v and the scan's words
  }
  if (divisor != 1.0f) {
#pragma unroll
    for (int k = 0; k < kIncPer; ++k) acc[k] = acc[k] / divisor;
  }
  store_vals<O>(out, e0, n, aligned && e0 + kIncPer <= n, acc);
}

// ------------------------------------------------------------------------------------------------
// the world-1 step: out = d(x), 16 B a lane
template <typename E>
__global__ __launch_bounds__(kIncBlock) void inc_step_e(const E* __restrict__ x, int64_t n, uint32_t lo, uint32_t mid,
                                                        E* __restrict__ out, int aligned) {
  constexpr int G = IncE<E>::G;
  const int64_t ng = (n + G - 1) / G;
#pragma unroll 2
  for (int64_t g = (int64_t)blockIdx.x * kIncBlock + threadIdx.x; g < ng; g += (int64_t)gridDim.x * kIncBlock) {
    const int64_t e = g * G;
    const bool fast = aligned && e + G <= n;
    uint32_t u[G];
    float d[G];
    load_bits<E>(x, e, n, fast, u);
#pragma unroll
    for (int j = 0; j < G; ++j) d[j] = u2f(inc_round_trip(u[j], lo, mid));
    store_vals<E>(out, e, n, fast, d);
  }
}

// ------------------------------------------------------------------------------------------------
// host side: one typed launcher per f32 / bf16 pair
static inline bool inc_shape_ok(int64_t n, int32_t b) { return n >= 0 && n < ((int64_t)1 << 31) && b >= 1 && b <= 14; }
static inline uint32_t inc_lo(int32_t b) { return (uint32_t)(127 - b); }
static inline uint32_t inc_mid(int32_t b) { return (uint32_t)(127 - b + (b + 1) / 2); }

template <typename E>
static grace_status_t inc_compress(const char* name, const char* bad, const E* x, int64_t n, int32_t b, uint8_t* payload,
                                   void* stream) {
  GRACE_REQUIRE(x && payload && inc_shape_ok(n, b) && IncE<E>::addressable(x) && al16(payload), bad);
  if (n == 0) return GRACE_OK;
  const hipStream_t st = as_stream(stream);
  const unsigned ntiles = (unsigned)inc_tiles(n);
  inc_init<<<1, kWave, 0, st>>>(reinterpret_cast<uint32_t*>(payload), ntiles);
  GRACE_CHECK_LAUNCH(name);
  inc_encode_e<E><<<ntiles, kIncBlock, 0, st>>>(x, n, inc_lo(b), inc_mid(b), payload, al16(x) ? 1 : 0);
  GRACE_CHECK_LAUNCH(name);
  return GRACE_OK;
}

template <typename E>
static grace_status_t inc_step(const char* name, const char* bad, const E* x, int64_t n, int32_t b, E* out, void* stream) {
  GRACE_REQUIRE(x && out && inc_shape_ok(n, b) && IncE<E>::addressable(x) && IncE<E>::addressable(out), bad);
  if (n == 0) return GRACE_OK;
  constexpr int G = IncE<E>::G;
  const unsigned grid = stream_grid((n + G - 1) / G, kIncBlock, kIncStepGridCap);
  inc_step_e<E><<<grid, kIncBlock, 0, as_stream(stream)>>>(x, n, inc_lo(b), inc_mid(b), out, al16(x) && al16(out) ? 1 : 0);
  GRACE_CHECK_LAUNCH(name);
  return GRACE_OK;
}

template <typename O>
static grace_status_t inc_decode(const char* name, const char* bad, const uint8_t* payloads, int64_t stride, int32_t world,
                                 int64_t n, int32_t b, float divisor, O* out, void* stream) {
  GRACE_REQUIRE(payloads && out && world >= 1 && world <= 1024 && inc_shape_ok(n, b) && divisor != 0.0f && stride >= 0 &&
                    stride % 16 == 0 && (n == 0 || stride >= 16 * inc_header_units(n)) && al16(payloads) &&
                    IncE<O>::addressable(out),
                bad);
  if (n == 0) return GRACE_OK;
  const float scale8 = __builtin_ldexpf(1.0f, (int)inc_mid(b) - 134);      // 2^-s8
  inc_decode_e<O><<<(unsigned)inc_tiles(n), kIncBlock, 0, as_stream(stream)>>>(
      payloads, stride, world, n, (uint32_t)inc_header_units(n), scale8, divisor, out, al16(out) ? 1 : 0);
  GRACE_CHECK_LAUNCH(name);
  return GRACE_OK;
}

}  // namespace grace

using namespace grace;

extern "C" {

size_t grace_inceptionn_capacity_bytes(int64_t n) {
  if (n <= 0 || n >= ((int64_t)1 << 31)) return 0;
  const int64_t full = n / kIncTile, m = n % kIncTile;
  return (size_t)(16 * inc_header_units(n) + full * (kIncTagBytes + kIncValBytes) +
                  (m ? 16 * ((m + 63) / 64) + 16 * ((m + 3) / 4) : 0));
}

grace_status_t grace_inceptionn_compress(const float* x, int64_t n, int32_t b, uint8_t* payload, void* stream) {
  return inc_compress<float>("grace_inceptionn_compress", "grace_inceptionn_compress: bad arguments", x, n, b, payload,
                             stream);
}

grace_status_t grace_inceptionn_compress_bf16(const uint16_t* x, int64_t n, int32_t b, uint8_t* payload,
                                              void* stream) {
  return inc_compress<uint16_t>("grace_inceptionn_compress_bf16", "grace_inceptionn_compress_bf16: bad arguments", x, n,
                                b, payload, stream);
}

grace_status_t grace_inceptionn_step_w1(const float* x, int64_t n, int32_t b, float* out, void* stream) {
  return inc_step<float>("grace_inceptionn_step_w1", "grace_inceptionn_step_w1: bad arguments", x, n, b, out, stream);
}

grace_status_t grace_inceptionn_step_w1_bf16(const uint16_t* x, int64_t n, int32_t b, uint16_t* out, void* stream) {
  return inc_step<uint16_t>("grace_inceptionn_step_w1_bf16", "grace_inceptionn_step_w1_bf16: bad arguments", x, n, b,
                            out, stream);
}

grace_status_t grace_inceptionn_decode_aggregate(const uint8_t* payloads, int64_t stride_bytes, int32_t world,
                                                 int64_t n, int32_t b, float divisor, float* out, void* stream) {
  return inc_decode<float>("grace_inceptionn_decode_aggregate", "grace_inceptionn_decode_aggregate: bad arguments",
                           payloads, stride_bytes, world, n, b, divisor, out, stream);
}

grace_status_t grace_inceptionn_decode_aggregate_bf16(const uint8_t* payloads, int64_t stride_bytes, int32_t world,
                                                      int64_t n, int32_t b, float divisor, uint16_t* out,
                                                      void* stream) {
  return inc_decode<uint16_t>("grace_inceptionn_decode_aggregate_bf16",
                              "grace_inceptionn_decode_aggregate_bf16: bad arguments", payloads, stride_bytes, world, n,
                              b, divisor, out, stream);
}

}  // extern "C"
