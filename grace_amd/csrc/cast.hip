// Natural compression (both flavours), fp16 and one-bit on bfloat16 gradients.
//
// Every kernel here is templated on the element type E of the gradient or of the dense result:
// float, or uint16_t holding the 16 bits of a bfloat16.  A bf16 gradient is widened exactly on load
// and a bf16 dense result is rounded once on store (common.h); the codes, the f16 payload, the means
// and every f32 in between come from the functions of codec.h, the ones the f32 kernels of quant.hip
// and elementwise.hip call.
//
// A lane handles one group of G consecutive elements per trip, G = 16 B of E (8 bf16, 4 f32): one
// 16-B load of the gradient, one 16-B store of a dense result, G bytes of codes.  The device
// generators stay keyed per quad at the quad's first index, so a group of 8 runs two quads' streams.
// A group that crosses n, or any group when an operand is not aligned for its vector access, goes
// through guarded per-element accesses in the same kernel: nothing outside [0, n) is touched.
//
// One-bit is new for both element types: encode in one pass over x (mask0 and f64 partials per
// workgroup, then a one-workgroup finish), the world-1 step in two passes (partials; then every
// workgroup sums the partials in one fixed order and writes its share of the result), the W-rank
// decode in one launch.  No kernel waits on another workgroup.
#include "common.h"
#include "codec.h"

#include "../../include/grace_hip_cast.h"

namespace grace {

constexpr int kCBlock = 256;
constexpr int kCGridCap = 4096;   // streaming kernels: workgroups at most
constexpr int kObParts = 1024;    // one-bit: workgroups (= f64 partials per sum) at most; 3 * kObParts doubles
                                  // fit grace_reduce_workspace_bytes (checked at launch)

// ------------------------------------------------------------------------------------------------
// Element access: a group is one 16-B load or store.
template <typename E>
struct Vec;

template <>
struct Vec<float> {
  static constexpr int G = 4;
  static bool aligned(const void* p) { return al16(p); }
  static bool addressable(const void* p) { return al4(p); }
  static __device__ __forceinline__ void ldv(const float* p, int64_t e, float (&v)[4]) {
    const float4 t = *reinterpret_cast<const float4*>(p + e);
    v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
  }
  static __device__ __forceinline__ float ld(const float* p, int64_t i) { return p[i]; }
  static __device__ __forceinline__ void stv(float* p, int64_t e, const float (&v)[4]) {
    *reinterpret_cast<float4*>(p + e) = make_float4(v[0], v[1], v[2], v[3]);
  }
  static __device__ __forceinline__ void st(float* p, int64_t i, float v) { p[i] = v; }
};

template <>
struct Vec<uint16_t> {
  static constexpr int G = 8;
  static bool aligned(const void* p) { return al16(p); }
  static bool addressable(const void* p) { return al2(p); }
  static __device__ __forceinline__ void ldv(const uint16_t* p, int64_t e, float (&v)[8]) {
    const uint4 t = *reinterpret_cast<const uint4*>(p + e);
    v[0] = u2f(t.x << 16); v[1] = u2f(t.x & 0xFFFF0000u); v[2] = u2f(t.y << 16); v[3] = u2f(t.y & 0xFFFF0000u);
    v[4] = u2f(t.z << 16); v[5] = u2f(t.z & 0xFFFF0000u); v[6] = u2f(t.w << 16); v[7] = u2f(t.w & 0xFFFF0000u);
  }
  static __device__ __forceinline__ float ld(const uint16_t* p, int64_t i) { return bf16_to_f32(p[i]); }
  static __device__ __forceinline__ void stv(uint16_t* p, int64_t e, const float (&v)[8]) {
    *reinterpret_cast<uint4*>(p + e) = make_uint4(pack_bf16x2(v[0], v[1]), pack_bf16x2(v[2], v[3]),
                                                  pack_bf16x2(v[4], v[5]), pack_bf16x2(v[6], v[7]));
  }
  static __device__ __forceinline__ void st(uint16_t* p, int64_t i, float v) { p[i] = f32_to_bf16(v); }
};

template <typename E>
__device__ __forceinline__ void load_group(const E* p, int64_t e, int64_t n, bool fast, float (&v)[Vec<E>::G]) {
  if (fast) {
    Vec<E>::ldv(p, e, v);
  } else {
#pragma unroll
    for (int j = 0; j < Vec<E>::G; ++j) v[j] = e + j < n ? Vec<E>::ld(p, e + j) : 0.f;
  }
}

template <typename E>
__device__ __forceinline__ void store_group(E* p, int64_t e, int64_t n, bool fast, const float (&v)[Vec<E>::G]) {
  if (fast) {
    Vec<E>::stv(p, e, v);
  } else {
#pragma unroll
    for (int j = 0; j < Vec<E>::G; ++j)
      if (e + j < n) Vec<E>::st(p, e + j, v[j]);
  }
}

// G injected randoms (f32 or i32) for the group: 16-B loads on the fast path, `fill` past n
template <int G, typename T>
__device__ __forceinline__ void load_rand(const T* p, int64_t e, int64_t n, bool fast, T fill, T (&r)[G]) {
  if (fast) {
#pragma unroll
    for (int q = 0; q < G / 4; ++q) {
      const uint4 t = *reinterpret_cast<const uint4*>(p + e + 4 * q);
      const uint32_t w[4] = {t.x, t.y, t.z, t.w};
#pragma unroll
      for (int j = 0; j < 4; ++j) __builtin_memcpy(&r[4 * q + j], &w[j], 4);
    }
  } else {
#pragma unroll
    for (int j = 0; j < G; ++j) r[j] = e + j < n ? p[e + j] : fill;
  }
}

__device__ __forceinline__ uint32_t pack_u8x4(const uint32_t* b) {
  return b[0] | (b[1] << 8) | (b[2] << 16) | (b[3] << 24);
}

// G u8 codes: one 4-B (G = 4) or 8-B (G = 8) access on the fast path
template <int G>
__device__ __forceinline__ void store_bytes(uint8_t* c, int64_t e, int64_t n, bool fast, const uint32_t (&b)[G]) {
  if (fast) {
    if constexpr (G == 4) *reinterpret_cast<uint32_t*>(c + e) = pack_u8x4(b);
    else *reinterpret_cast<uint2*>(c + e) = make_uint2(pack_u8x4(b), pack_u8x4(b + 4));
  } else {
#pragma unroll
    for (int j = 0; j < G; ++j)
      if (e + j < n) c[e + j] = (uint8_t)b[j];
  }
}

template <int G>
__device__ __forceinline__ void load_bytes(const uint8_t* c, int64_t e, int64_t n, bool fast, uint32_t (&b)[G]) {
  if (fast) {
    uint32_t w[G / 4];
    if constexpr (G == 4) {
      w[0] = *reinterpret_cast<const uint32_t*>(c + e);
    } else {
      const uint2 t = *reinterpret_cast<const uint2*>(c + e);
      w[0] = t.x; w[1] = t.y;
    }
#pragma unroll
    for (int j = 0; j < G; ++j) b[j] = (w[j >> 2] >> (8 * (j & 3))) & 0xFFu;
  } else {
#pragma unroll
    for (int j = 0; j < G; ++j) b[j] = e + j < n ? (uint32_t)c[e + j] : 0u;
  }
}

// G 16-bit patterns (the f16 payload): one 8-B (G = 4) or 16-B (G = 8) access on the fast path
template <int G>
__device__ __forceinline__ void store_halves(uint16_t* h, int64_t e, int64_t n, bool fast, const uint32_t (&b)[G]) {
  if (fast) {
    if constexpr (G == 4) {
      *reinterpret_cast<uint2*>(h + e) = make_uint2(b[0] | (b[1] << 16), b[2] | (b[3] << 16));
    } else {
      *reinterpret_cast<uint4*>(h + e) =
          make_uint4(b[0] | (b[1] << 16), b[2] | (b[3] << 16), b[4] | (b[5] << 16), b[6] | (b[7] << 16));
    }
  } else {
#pragma unroll
    for (int j = 0; j < G; ++j)
      if (e + j < n) h[e + j] = (uint16_t)b[j];
  }
}

template <int G>
__device__ __forceinline__ void load_halves(const uint16_t* h, int64_t e, int64_t n, bool fast, uint32_t (&b)[G]) {
  if (fast) {
    uint32_t w[G / 2];
    if constexpr (G == 4) {
      const uint2 t = *reinterpret_cast<const uint2*>(h + e);
      w[0] = t.x; w[1] = t.y;
    } else {
      const uint4 t = *reinterpret_cast<const uint4*>(h + e);
      w[0] = t.x; w[1] = t.y; w[2] = t.z; w[3] = t.w;
    }
#pragma unroll
    for (int j = 0; j < G; ++j) b[j] = (w[j >> 1] >> (16 * (j & 1))) & 0xFFFFu;
  } else {
#pragma unroll
    for (int j = 0; j < G; ++j) b[j] = e + j < n ? (uint32_t)h[e + j] : 0u;
  }
}

// the device generators of the group's quads, each keyed at its first index (+ xoff)
template <int G>
__device__ __forceinline__ void natural_rand_group(uint64_t seed, int64_t e, int32_t (&r)[G]) {
#pragma unroll
  for (int q = 0; q < G / 4; ++q) {
    int32_t t[4];
    natural_rand4(seed, e + 4 * q, t);
#pragma unroll
    for (int j = 0; j < 4; ++j) r[4 * q + j] = t[j];
  }
}
template <int G>
__device__ __forceinline__ void uniform_group(uint64_t seed, int64_t e, float (&u)[G]) {
#pragma unroll
  for (int q = 0; q < G / 4; ++q) {
    float t[4];
    uniform01x4(seed, (uint64_t)(e + 4 * q), t);
#pragma unroll
    for (int j = 0; j < 4; ++j) u[4 * q + j] = t[j];
  }
}

#define GRACE_GROUP_LOOP(E)                                                                                   \
  constexpr int G = Vec<E>::G;                                                                                \
  const int64_t ng = (n + G - 1) / G;                                                                         \
  for (int64_t g = (int64_t)blockIdx.x * kCBlock + threadIdx.x; g < ng; g += (int64_t)gridDim.x * kCBlock)

// ------------------------------------------------------------------------------------------------
// encoders (quant.hip's natural_encode_kernel, cnat_encode_kernel, f32_to_f16_kernel on E)
template <typename E>
__global__ __launch_bounds__(kCBlock) void natural_encode_e(const E* __restrict__ x, int64_t n,
                                                            const int32_t* __restrict__ ri, uint64_t seed,
                                                            uint8_t* __restrict__ codes, int aligned, int64_t xoff) {
  GRACE_GROUP_LOOP(E) {
    const int64_t e = g * G;
    const bool fast = aligned && e + G - 1 < n;
    float v[G];
    int32_t r[G];
    load_group<E>(x, e, n, fast, v);
    if (ri) load_rand<G, int32_t>(ri, e, n, fast, 0, r);
    else natural_rand_group<G>(seed, e + xoff, r);
    uint32_t c[G];
#pragma unroll
    for (int j = 0; j < G; ++j) c[j] = natural_code(v[j], r[j]);
    store_bytes<G>(codes, e, n, fast, c);
  }
}

template <typename E>
__global__ __launch_bounds__(kCBlock) void cnat_encode_e(const E* __restrict__ x, int64_t n,
                                                         const float* __restrict__ rnd, int deterministic,
                                                         uint64_t seed, uint8_t* __restrict__ codes, int aligned,
                                                         int64_t xoff) {
  GRACE_GROUP_LOOP(E) {
    const int64_t e = g * G;
    const bool fast = aligned && e + G - 1 < n;
    float v[G], r[G];
    load_group<E>(x, e, n, fast, v);
    if (deterministic) {
#pragma unroll
      for (int j = 0; j < G; ++j) r[j] = 0.5f;
    } else if (rnd) {
      load_rand<G, float>(rnd, e, n, fast, 0.f, r);
    } else {
      uniform_group<G>(seed, e + xoff, r);
    }
    uint32_t c[G];
#pragma unroll
    for (int j = 0; j < G; ++j) c[j] = cnat_code(v[j], r[j]);
    store_bytes<G>(codes, e, n, fast, c);
  }
}

template <typename E>
__global__ __launch_bounds__(kCBlock) void f16_encode_e(const E* __restrict__ x, uint16_t* __restrict__ h, int64_t n,
                                                        int aligned) {
  GRACE_GROUP_LOOP(E) {
    const int64_t e = g * G;
    const bool fast = aligned && e + G - 1 < n;
    float v[G];
    load_group<E>(x, e, n, fast, v);
    uint32_t b[G];
#pragma unroll
    for (int j = 0; j < G; ++j) b[j] = f16_bits(v[j]);
    store_halves<G>(h, e, n, fast, b);
  }
}

// world-1 step in one pass: out = 0 + dec(enc(x)), the codes never stored (cast_step_w1_kernel on E)
template <int MODE, typename E>
__global__ __launch_bounds__(kCBlock) void cast_step_e(const E* __restrict__ x, E* __restrict__ o, int64_t n,
                                                       uint64_t seed, int aligned) {
  GRACE_GROUP_LOOP(E) {
    const int64_t e = g * G;
    const bool fast = aligned && e + G - 1 < n;
    float v[G], u[G];
    int32_t r[G];
    load_group<E>(x, e, n, fast, v);
#pragma unroll
    for (int j = 0; j < G; ++j) { u[j] = 0.5f; r[j] = 0; }
    if constexpr (MODE == kCastNatural) natural_rand_group<G>(seed, e, r);
    if constexpr (MODE == kCastCnat) uniform_group<G>(seed, e, u);
    float d[G];
#pragma unroll
    for (int j = 0; j < G; ++j) d[j] = cast_round_trip<MODE>(v[j], u[j], r[j]);
    store_group<E>(o, e, n, fast, d);
  }
}

// ------------------------------------------------------------------------------------------------
// decoders: W rank-major payloads at `stride`, summed in rank order, one division, one rounding
template <int FLAVOUR, typename E>
__global__ __launch_bounds__(kCBlock) void natural_decode_e(const uint8_t* __restrict__ codes, int64_t stride,
                                                            int world, int64_t n, float divisor, int aggregate,
                                                            E* __restrict__ out, int aligned) {
  GRACE_GROUP_LOOP(E) {
    const int64_t e = g * G;
    const bool fast = aligned && e + G - 1 < n;
    float acc[G];
#pragma unroll
    for (int j = 0; j < G; ++j) acc[j] = 0.f;
    for (int w = 0; w < world; ++w) {
      uint32_t c[G];
      load_bytes<G>(codes + w * stride, e, n, fast, c);
#pragma unroll
      for (int j = 0; j < G; ++j) {
        const float d = FLAVOUR == 0 ? natural_dec(c[j]) : cnat_dec(c[j]);
        acc[j] = (aggregate || w > 0) ? acc[j] + d : d;
      }
    }
#pragma unroll
    for (int j = 0; j < G; ++j) acc[j] = divisor == 1.0f ? acc[j] : acc[j] / divisor;
    store_group<E>(out, e, n, fast, acc);
  }
}

template <typename E>
__global__ __launch_bounds__(kCBlock) void f16_decode_e(const uint16_t* __restrict__ h, int64_t stride, int world,
                                                        int64_t n, float divisor, E* __restrict__ out, int aligned) {
  GRACE_GROUP_LOOP(E) {
    const int64_t e = g * G;
    const bool fast = aligned && e + G - 1 < n;
    float acc[G];
#pragma unroll
    for (int j = 0; j < G; ++j) acc[j] = 0.f;
    for (int w = 0; w < world; ++w) {
      uint32_t b[G];
      load_halves<G>(h + w * stride, e, n, fast, b);
#pragma unroll
      for (int j = 0; j < G; ++j) acc[j] = acc[j] + f16_value(b[j]);
    }
#pragma unroll
    for (int j = 0; j < G; ++j) acc[j] = divisor == 1.0f ? acc[j] : acc[j] / divisor;
    store_group<E>(out, e, n, fast, acc);
  }
}

// ------------------------------------------------------------------------------------------------
// one-bit
struct ObSums { double sum0, num0, sum1; };

// Sums over the workgroup, the same bits in every thread: xor butterflies inside each wave, then the
// wave totals in wave order.  Called once per kernel (one LDS array, no reuse hazard).
__device__ __forceinline__ ObSums block_sum3(ObSums v) {
  __shared__ double sh[3][kCBlock / kWave];
  v.sum0 = wave_sum(v.sum0); v.num0 = wave_sum(v.num0); v.sum1 = wave_sum(v.sum1);
  if ((threadIdx.x & 63) == 0) {
    sh[0][threadIdx.x >> 6] = v.sum0; sh[1][threadIdx.x >> 6] = v.num0; sh[2][threadIdx.x >> 6] = v.sum1;
  }
  __syncthreads();
  ObSums t{0.0, 0.0, 0.0};
#pragma unroll
  for (int w = 0; w < kCBlock / kWave; ++w) { t.sum0 += sh[0][w]; t.num0 += sh[1][w]; t.sum1 += sh[2][w]; }
  return t;
}

// The totals of the partials, in one fixed order whatever workgroup runs it: thread t adds partials
// t, t + 256, ... in turn, then block_sum3.  part[j * nparts + b] is sum j of workgroup b.
__device__ __forceinline__ ObSums sum_parts(const double* __restrict__ part, int nparts) {
  ObSums s{0.0, 0.0, 0.0};
  for (int b = threadIdx.x; b < nparts; b += kCBlock) {
    s.sum0 += part[b]; s.num0 += part[nparts + b]; s.sum1 += part[2 * nparts + b];
  }
  return block_sum3(s);
}

// Pass over x: mask0 = (x < 0) when mask0 is given, and the workgroup's f64 partials (sum over
// x < 0, their count, sum over the rest -- NaN is "not x < 0").  The partition and the order of every
// addition depend only on (n, the grid, the path), so two calls give the same bits.
template <typename E>
__global__ __launch_bounds__(kCBlock) void onebit_sums_e(const E* __restrict__ x, int64_t n,
                                                         uint8_t* __restrict__ mask0, double* __restrict__ part,
                                                         int aligned) {
  ObSums s{0.0, 0.0, 0.0};
  uint32_t cnt = 0;   // a lane sees fewer than 2^32 elements of a bucket below 2^40
  GRACE_GROUP_LOOP(E) {
    const int64_t e = g * G;
    const bool fast = aligned && e + G - 1 < n;
    float v[G];
    load_group<E>(x, e, n, fast, v);
    uint32_t b[G];
#pragma unroll
    for (int j = 0; j < G; ++j) {
      b[j] = (uint32_t)(v[j] < 0.f);
      if (fast || e + j < n) {
        if (b[j]) { s.sum0 += (double)v[j]; ++cnt; } else { s.sum1 += (double)v[j]; }
      }
    }
    if (mask0) store_bytes<G>(mask0, e, n, fast, b);
  }
  s.num0 = (double)cnt;
  s = block_sum3(s);
  if (threadIdx.x == 0) {
    part[blockIdx.x] = s.sum0;
    part[gridDim.x + blockIdx.x] = s.num0;
    part[2 * gridDim.x + blockIdx.x] = s.sum1;
  }
}

__global__ __launch_bounds__(kCBlock) void onebit_finish_kernel(const double* __restrict__ part, int nparts, int64_t n,
                                                                float* __restrict__ means) {
  const ObSums t = sum_parts(part, nparts);
  if (threadIdx.x == 0) onebit_means(t.sum0, t.num0, t.sum1, n, means);
}

// Pass B of the world-1 step: every workgroup forms the means from the partials (workgroup 0 stores
// them), each lane forms the two decoded values 0 + dec(1) and 0 + dec(0) once and selects per element.
template <typename E>
__global__ __launch_bounds__(kCBlock) void onebit_apply_e(const E* __restrict__ x, int64_t n,
                                                          const double* __restrict__ part, int nparts,
                                                          float* __restrict__ means, int quirk, E* __restrict__ out,
                                                          int aligned) {
  const ObSums t = sum_parts(part, nparts);
  float m[2];
  onebit_means(t.sum0, t.num0, t.sum1, n, m);
  if (blockIdx.x == 0 && threadIdx.x == 0) { means[0] = m[0]; means[1] = m[1]; }
  const float d_neg = 0.f + onebit_dec(1u, m[0], m[1], quirk);
  const float d_rest = 0.f + onebit_dec(0u, m[0], m[1], quirk);
  GRACE_GROUP_LOOP(E) {
    const int64_t e = g * G;
    const bool fast = aligned && e + G - 1 < n;
    float v[G];
    load_group<E>(x, e, n, fast, v);
#pragma unroll
    for (int j = 0; j < G; ++j) v[j] = v[j] < 0.f ? d_neg : d_rest;
    store_group<E>(out, e, n, fast, v);
  }
}

// out = (((0 + d_0) + d_1) + ...) / divisor over W gathered payloads, rank w's mask0 at + w * n
template <typename E>
__global__ __launch_bounds__(kCBlock) void onebit_decode_e(const uint8_t* __restrict__ mask_wn,
                                                           const float* __restrict__ mean0,
                                                           const float* __restrict__ mean1, int world, int quirk,
                                                           float divisor, E* __restrict__ out, int64_t n, int aligned) {
  GRACE_GROUP_LOOP(E) {
    const int64_t e = g * G;
    const bool fast = aligned && e + G - 1 < n;
    float acc[G];
#pragma unroll
    for (int j = 0; j < G; ++j) acc[j] = 0.f;
    for (int w = 0; w < world; ++w) {
      const float m0 = mean0[w], m1 = mean1[w];
      uint32_t b[G];
      load_bytes<G>(mask_wn + (int64_t)w * n, e, n, fast, b);
#pragma unroll
      for (int j = 0; j < G; ++j) acc[j] = acc[j] + onebit_dec(b[j], m0, m1, quirk);
    }
#pragma unroll
    for (int j = 0; j < G; ++j) acc[j] = divisor == 1.0f ? acc[j] : acc[j] / divisor;
    store_group<E>(out, e, n, fast, acc);
  }
}

// ------------------------------------------------------------------------------------------------
// host side: one typed launcher per f32 / bf16 pair
template <typename E>
static inline unsigned group_grid(int64_t n, int64_t cap) {
  return stream_grid((n + Vec<E>::G - 1) / Vec<E>::G, kCBlock, cap);
}
// whether the u8 row(s) allow one G-byte access per group
template <typename E>
static inline bool bytes_aligned(const void* p) { return Vec<E>::G == 8 ? al8(p) : al4(p); }

template <typename E>
static grace_status_t onebit_encode(const char* name, const char* bad, const E* x, int64_t n, uint8_t* mask0,
                                    float* means, void* ws, void* stream) {
  GRACE_REQUIRE(n > 0 && x && mask0 && means && ws && Vec<E>::addressable(x) && al8(ws) && al4(means) &&
                    sizeof(double) * 3 * kObParts <= grace_reduce_workspace_bytes(n),
                bad);
  const int al = Vec<E>::aligned(x) && bytes_aligned<E>(mask0);
  const unsigned grid = group_grid<E>(n, kObParts);
  double* part = reinterpret_cast<double*>(ws);
  onebit_sums_e<E><<<grid, kCBlock, 0, as_stream(stream)>>>(x, n, mask0, part, al);
  GRACE_CHECK_LAUNCH(name);
  onebit_finish_kernel<<<1, kCBlock, 0, as_stream(stream)>>>(part, (int)grid, n, means);
  GRACE_CHECK_LAUNCH(name);
  return GRACE_OK;
}

template <typename E>
static grace_status_t onebit_step(const char* name, const char* bad, const E* x, int64_t n, int32_t quirk, float* means,
                                  E* out, void* ws, void* stream) {
  GRACE_REQUIRE(n > 0 && x && means && out && ws && Vec<E>::addressable(x) && Vec<E>::addressable(out) && al8(ws) &&
                    al4(means) && sizeof(double) * 3 * kObParts <= grace_reduce_workspace_bytes(n),
                bad);
  const int al = Vec<E>::aligned(x) && Vec<E>::aligned(out);
  const unsigned grid = group_grid<E>(n, kObParts);
  double* part = reinterpret_cast<double*>(ws);
  onebit_sums_e<E><<<grid, kCBlock, 0, as_stream(stream)>>>(x, n, nullptr, part, Vec<E>::aligned(x) ? 1 : 0);
  GRACE_CHECK_LAUNCH(name);
  onebit_apply_e<E><<<grid, kCBlock, 0, as_stream(stream)>>>(x, n, part, (int)grid, means, quirk ? 1 : 0, out, al);
  GRACE_CHECK_LAUNCH(name);
  return GRACE_OK;
}

template <typename E>
static grace_status_t onebit_decode(const char* name, const char* bad, const uint8_t* mask_wn, const float* mean0,
                                    const float* mean1, int32_t world, int32_t quirk, float divisor, E* out, int64_t n,
                                    void* stream) {
  GRACE_REQUIRE(mask_wn && mean0 && mean1 && out && world >= 1 && n >= 0 && divisor != 0.0f && al4(mean0) &&
                    al4(mean1) && Vec<E>::addressable(out),
                bad);
  if (n == 0) return GRACE_OK;
  const int al = bytes_aligned<E>(mask_wn) && (world == 1 || n % Vec<E>::G == 0) && Vec<E>::aligned(out);
  onebit_decode_e<E><<<group_grid<E>(n, kCGridCap), kCBlock, 0, as_stream(stream)>>>(mask_wn, mean0, mean1, world,
                                                                                    quirk ? 1 : 0, divisor, out, n, al);
  GRACE_CHECK_LAUNCH(name);
  return GRACE_OK;
}

}  // namespace grace

using namespace grace;
typedef uint16_t bf16_t;

extern "C" {

grace_status_t grace_natural_compress_at_bf16(const uint16_t* x, int64_t xoff, int64_t n, const int32_t* rand_int,
                                              uint64_t seed, uint8_t* codes, void* stream) {
  GRACE_REQUIRE(x && codes && n >= 0 && xoff >= 0 && (xoff & 3) == 0 && al2(x) && al4(rand_int),
                "grace_natural_compress_at_bf16: bad arguments");
  if (n == 0) return GRACE_OK;
  const int al = al16(x) && al16(rand_int) && al8(codes);
  natural_encode_e<bf16_t><<<group_grid<bf16_t>(n, kCGridCap), kCBlock, 0, as_stream(stream)>>>(x, n, rand_int, seed,
                                                                                               codes, al, xoff);
  GRACE_CHECK_LAUNCH("grace_natural_compress_at_bf16");
  return GRACE_OK;
}

grace_status_t grace_cnat_compress_at_bf16(const uint16_t* x, int64_t xoff, int64_t n, const float* rand,
                                           int32_t deterministic, uint64_t seed, uint8_t* codes, void* stream) {
  GRACE_REQUIRE(x && codes && n >= 0 && xoff >= 0 && (xoff & 3) == 0 && al2(x) && al4(rand),
                "grace_cnat_compress_at_bf16: bad arguments");
  if (n == 0) return GRACE_OK;
  const int al = al16(x) && al16(rand) && al8(codes);
  cnat_encode_e<bf16_t><<<group_grid<bf16_t>(n, kCGridCap), kCBlock, 0, as_stream(stream)>>>(
      x, n, rand, deterministic, seed, codes, al, xoff);
  GRACE_CHECK_LAUNCH("grace_cnat_compress_at_bf16");
  return GRACE_OK;
}

grace_status_t grace_fp16_compress_bf16(const uint16_t* x, void* half_out, int64_t n, void* stream) {
  GRACE_REQUIRE(x && half_out && n >= 0 && al2(x) && al2(half_out), "grace_fp16_compress_bf16: bad arguments");
  if (n == 0) return GRACE_OK;
  const int al = al16(x) && al16(half_out);
  f16_encode_e<bf16_t><<<group_grid<bf16_t>(n, kCGridCap), kCBlock, 0, as_stream(stream)>>>(
      x, reinterpret_cast<uint16_t*>(half_out), n, al);
  GRACE_CHECK_LAUNCH("grace_fp16_compress_bf16");
  return GRACE_OK;
}

grace_status_t grace_cast_step_w1_bf16(const uint16_t* x, int64_t n, int32_t mode, uint64_t seed, uint16_t* out,
                                       void* stream) {
  GRACE_REQUIRE(x && out && n >= 0 && mode >= 0 && mode <= 3 && al2(x) && al2(out),
                "grace_cast_step_w1_bf16: bad arguments");
  if (n == 0) return GRACE_OK;
  const int al = al16(x) && al16(out);
  const unsigned grid = group_grid<bf16_t>(n, kCGridCap);
  const hipStream_t st = as_stream(stream);
  switch (mode) {
    case kCastNatural: cast_step_e<kCastNatural, bf16_t><<<grid, kCBlock, 0, st>>>(x, out, n, seed, al); break;
    case kCastCnat: cast_step_e<kCastCnat, bf16_t><<<grid, kCBlock, 0, st>>>(x, out, n, seed, al); break;
    case kCastCnatDet: cast_step_e<kCastCnatDet, bf16_t><<<grid, kCBlock, 0, st>>>(x, out, n, seed, al); break;
    default: cast_step_e<kCastF16, bf16_t><<<grid, kCBlock, 0, st>>>(x, out, n, seed, al); break;
  }
  GRACE_CHECK_LAUNCH("grace_cast_step_w1_bf16");
  return GRACE_OK;
}

grace_status_t grace_natural_decompress_bf16(const uint8_t* codes, int64_t stride, int32_t world, int64_t n,
                                             int32_t flavour, int32_t aggregate, float divisor, uint16_t* out,
                                             void* stream) {
  GRACE_REQUIRE(codes && out && world >= 1 && n >= 0 && (flavour == 0 || flavour == 1) && divisor != 0.0f &&
                    (world == 1 || stride >= n) && al2(out),
                "grace_natural_decompress_bf16: bad arguments");
  if (n == 0) return GRACE_OK;
  const unsigned grid = group_grid<bf16_t>(n, kCGridCap);
  const int al = al8(codes) && (stride % 8 == 0 || world == 1) && al16(out);
  if (flavour == 0)
    natural_decode_e<0, bf16_t><<<grid, kCBlock, 0, as_stream(stream)>>>(codes, stride, world, n, divisor, aggregate,
                                                                         out, al);
  else
    natural_decode_e<1, bf16_t><<<grid, kCBlock, 0, as_stream(stream)>>>(codes, stride, world, n, divisor, aggregate,
                                                                         out, al);
  GRACE_CHECK_LAUNCH("grace_natural_decompress_bf16");
  return GRACE_OK;
}

grace_status_t grace_fp16_decompress_aggregate_bf16(const void* half_in, int64_t stride, int32_t world, int64_t n,
                                                    float divisor, uint16_t* out, void* stream) {
  GRACE_REQUIRE(half_in && out && n >= 0 && world >= 1 && stride >= n && divisor != 0.0f && al2(half_in) && al2(out),
                "grace_fp16_decompress_aggregate_bf16: bad arguments");
  if (n == 0) return GRACE_OK;
  const int al = al16(half_in) && (stride % 8 == 0 || world == 1) && al16(out);
  f16_decode_e<bf16_t><<<group_grid<bf16_t>(n, kCGridCap), kCBlock, 0, as_stream(stream)>>>(
      reinterpret_cast<const uint16_t*>(half_in), stride, world, n, divisor, out, al);
  GRACE_CHECK_LAUNCH("grace_fp16_decompress_aggregate_bf16");
  return GRACE_OK;
}

grace_status_t grace_onebit_encode_bf16(const uint16_t* x, int64_t n, uint8_t* mask0, float* means_dev, void* ws,
                                        void* stream) {
  return onebit_encode<bf16_t>("grace_onebit_encode_bf16", "grace_onebit_encode_bf16: bad arguments", x, n, mask0,
                               means_dev, ws, stream);
}

grace_status_t grace_onebit_step_w1(const float* x, int64_t n, int32_t quirk, float* means_dev, float* out, void* ws,
                                    void* stream) {
  return onebit_step<float>("grace_onebit_step_w1", "grace_onebit_step_w1: bad arguments", x, n, quirk, means_dev, out,
                            ws, stream);
}

grace_status_t grace_onebit_step_w1_bf16(const uint16_t* x, int64_t n, int32_t quirk, float* means_dev, uint16_t* out,
                                         void* ws, void* stream) {
  return onebit_step<bf16_t>("grace_onebit_step_w1_bf16", "grace_onebit_step_w1_bf16: bad arguments", x, n, quirk,
                             means_dev, out, ws, stream);
}

grace_status_t grace_onebit_decode_aggregate(const uint8_t* mask0_wn, const float* mean0_w, const float* mean1_w,
                                             int32_t world, int32_t quirk, float divisor, float* out, int64_t n,
                                             void* stream) {
  return onebit_decode<float>("grace_onebit_decode_aggregate", "grace_onebit_decode_aggregate: bad arguments", mask0_wn,
                              mean0_w, mean1_w, world, quirk, divisor, out, n, stream);
}

grace_status_t grace_onebit_decode_aggregate_bf16(const uint8_t* mask0_wn, const float* mean0_w, const float* mean1_w,
                                                  int32_t world, int32_t quirk, float divisor, uint16_t* out, int64_t n,
                                                  void* stream) {
  return onebit_decode<bf16_t>("grace_onebit_decode_aggregate_bf16",
                               "grace_onebit_decode_aggregate_bf16: bad arguments", mask0_wn, mean0_w, mean1_w, world,
                               quirk, divisor, out, n, stream);
}

}  // extern "C"
