// The OCP Microscaling formats as a gradient codec (the arithmetic and the wire are stated
// in include/grace_hip_mx.h): blocks of 32 elements, one E8M0 scale byte a block, FP8 / FP6 / FP4 codes.
//
// Encode is one kernel template over <element type, format, stochastic, fused>.  A wave owns whole chunks
// of 1024 elements (32 blocks); a row is one 16-B load of every lane (64 * G elements: 256 f32, 512 bf16),
// so a chunk is 4 rows of f32 or 2 of bf16 and a block lives in 8 (f32) or 4 (bf16) neighbouring lanes of
// one row.  The lane keeps the raw 16-B words in registers; the block maximum is a DPP butterfly over those
// lanes (row8_max / quad_max: no LDS, no atomics), the conversion is integer work on the significands,
// and the loads of the wave's next chunk are issued before the current one is converted.
//
// A lane's codes of one row are an item of I = bits * G bits: 32 or 64 for FP8 and bf16 FP4 (stored as
// they are), 16 for f32 FP4, 24 for f32 FP6, 48 for bf16 FP6.  Those items are transposed over T = 2 or 4
// neighbouring lanes and as many rows by DPP quad permutes, so that lane q of the group holds row q's
// items of the whole group: T * I bits, 1 or 3 whole dwords, stored as one dword or dwordx3.  Row q's
// region follows row q - 1's, so one store instruction of a wave covers T * 64 * I / 8 contiguous bytes.
// The 32 scale bytes of a chunk are collected from the blocks' first lanes by v_readlane and leave lane 0
// as two 16-B stores.  A chunk that crosses n goes through guarded per-byte stores (whole blocks only,
// so every byte of the payload is written once), and x or out off the 16-B grid through guarded
// per-element accesses, all in the same kernel.
//
// Decode + aggregate gives a thread the elements of one (FP8, FP4) or three (FP6) 16-B lines of codes:
// 16, 32 or 64 elements and 1, 1 or 2 scale bytes a rank, summed over the ranks in registers and written
// as 16-B stores.
#include "common.h"

#include "../../include/grace_hip_mx.h"

namespace grace {

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef uint32_t u32x3v __attribute__((ext_vector_type(3)));
typedef u32x3v u32x3 __attribute__((aligned(4)));      // a dwordx3 store needs dword alignment only
typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));

constexpr int kMxBlock = 256;          // threads per workgroup: 4 waves
constexpr int kMxWaves = kMxBlock / kWave;
constexpr int kMxChunk = 1024;         // elements a wave converts per iteration: 32 blocks
constexpr int kMxGridCap = 512;        // encode: workgroups at most (a wave loops over its chunks)
constexpr int kMxDecGridCap = 4096;
constexpr uint32_t kMxNaN = 0x7FC00000u;

template <int F> struct MxF;
template <> struct MxF<0> { static constexpr int BITS = 8, MB = 3, BIAS = 7, EMAX = 8, MAXC = 0x7E; };
template <> struct MxF<1> { static constexpr int BITS = 8, MB = 2, BIAS = 15, EMAX = 15, MAXC = 0x7B; };
template <> struct MxF<2> { static constexpr int BITS = 6, MB = 3, BIAS = 1, EMAX = 2, MAXC = 0x1F; };
template <> struct MxF<3> { static constexpr int BITS = 6, MB = 2, BIAS = 3, EMAX = 4, MAXC = 0x1F; };
template <> struct MxF<4> { static constexpr int BITS = 4, MB = 1, BIAS = 1, EMAX = 2, MAXC = 0x7; };
static const int kMxBits[5] = {8, 8, 6, 6, 4};

static inline bool mx_format_ok(int32_t f) { return f >= 0 && f <= 4; }
static inline size_t ceil16(size_t x) { return (x + 15) & ~(size_t)15; }
static inline size_t mx_bytes(int64_t n, int32_t format) {
  const size_t nb = (size_t)((n + 31) >> 5);
  return ceil16(nb) + ceil16(nb * 4 * (size_t)kMxBits[format]);
}

// ------------------------------------------------------------------------------------------------
// Element access.  A lane's share of a row travels as the raw 16 B it was loaded as and is unpacked
// into f32 bit patterns.
template <typename E>
struct MxE;

template <>
struct MxE<float> {
  static constexpr int G = 4;
  static bool addressable(const void* p) { return al4(p); }
  static __device__ __forceinline__ void unpack(u32x4 t, uint32_t (&v)[4]) {
    v[0] = t[0]; v[1] = t[1]; v[2] = t[2]; v[3] = t[3];
  }
  static __device__ __forceinline__ u32x4 gather(const float* p, int64_t e, int64_t n) {
    u32x4 t;
#pragma unroll
    for (int j = 0; j < 4; ++j) t[j] = e + j < n ? f2u(p[e + j]) : 0u;
    return t;
  }
  static __device__ __forceinline__ void put(float* o, int64_t e, int64_t n, bool fast, const float (&d)[4]) {
    if (fast) {
      u32x4 t;
#pragma unroll
      for (int j = 0; j < 4; ++j) t[j] = f2u(d[j]);
      __builtin_nontemporal_store(t, reinterpret_cast<u32x4*>(o + e));
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (e + j < n) o[e + j] = d[j];
    }
  }
};

template <>
struct MxE<uint16_t> {
  static constexpr int G = 8;
  static bool addressable(const void* p) { return al2(p); }
  static __device__ __forceinline__ void unpack(u32x4 t, uint32_t (&v)[8]) {
#pragma unroll
    for (int k = 0; k < 4; ++k) { v[2 * k] = t[k] << 16; v[2 * k + 1] = t[k] & 0xFFFF0000u; }
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
  static __device__ __forceinline__ void put(uint16_t* o, int64_t e, int64_t n, bool fast, const float (&d)[8]) {
    if (fast) {
      u32x4 t;
#pragma unroll
      for (int k = 0; k < 4; ++k) t[k] = pack_bf16x2(d[2 * k], d[2 * k + 1]);
      __builtin_nontemporal_store(t, reinterpret_cast<u32x4*>(o + e));
    } else {
#pragma unroll
      for (int j = 0; j < 8; ++j)
        if (e + j < n) o[e + j] = f32_to_bf16(d[j]);
    }
  }
};

template <typename E>
__device__ __forceinline__ u32x4 mx_load(const E* x, int64_t e, int64_t n, bool fast) {
  if (fast) return __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(x + e));
  return MxE<E>::gather(x, e, n);
}

// ------------------------------------------------------------------------------------------------
// The conversion.  u: the f32 bits of x; e: the block's scale byte; k: the 24-bit uniform (SR only).
// |x| = sig * 2^(ex - 150) with sig in [2^23, 2^24) (a denormal is normalised; zero gives sig = 0), so
// y = sig * 2^(ex - e - 23) and the target's exponent field is ce = ex - e + bias when that is >= 1.
// lo's code is sig shifted right by sh (the target's subnormals shift further), r the bits shifted out.
template <int F, bool SR>
__device__ __forceinline__ uint32_t mx_code(uint32_t u, int e, uint32_t k) {
  using X = MxF<F>;
  const uint32_t ef = (u >> 23) & 0xFFu, m = u & 0x7FFFFFu;
  const int lz = ef ? 0 : __builtin_clz(m | 1u) - 8;
  const uint32_t sig = ef ? (m | 0x800000u) : (m << lz);
  const int ce = (ef ? (int)ef : 1 - lz) - e + X::BIAS;
  const int sh = (23 - X::MB) + (ce >= 1 ? 0 : 1 - ce);
  const int shc = min(sh, 31);                       // sig < 2^24: any shift past 24 leaves lo = 0, r = sig
  const uint32_t lo = (sig >> shc) + (ce >= 1 ? (uint32_t)(ce - 1) << X::MB : 0u);
  const uint32_t r = sig & ((1u << shc) - 1u);
  bool up;
  if constexpr (SR) {
    // u < r / 2^sh  <=>  k < ceil(r * 2^(24 - sh))
    const int d = max(min(sh, 55) - 24, 0);          // past 55 the ceiling is still (r != 0)
    const uint32_t t = sh <= 24 ? r << max(24 - sh, 0) : (r + (1u << d) - 1u) >> d;
    up = k < t;
  } else {
    const uint32_t half = 1u << (shc - 1);
    up = r > half || (r == half && (lo & 1u));
  }
  return min(lo + (up ? 1u : 0u), (uint32_t)X::MAXC) | ((u >> 31) << (X::BITS - 1));
}

// magnitude code -> its value as f32, exactly: the fields moved into place; a subnormal is
// (1 + f) 2^(1 - bias) - 2^(1 - bias)
template <int F>
__device__ __forceinline__ float mx_value(uint32_t mag) {
  using X = MxF<F>;
  const uint32_t base = (mag << (23 - X::MB)) + ((uint32_t)(127 - X::BIAS) << 23);
  float v = (mag >> X::MB) ? u2f(base) : u2f(base + (1u << 23)) - u2f((uint32_t)(128 - X::BIAS) << 23);
  if constexpr (F == 0) v = mag == 0x7Fu ? u2f(kMxNaN) : v;
  if constexpr (F == 1) v = mag >= 0x7Cu ? u2f(mag == 0x7Cu ? 0x7F800000u : kMxNaN) : v;
  return v;
}

template <int F>
__device__ __forceinline__ float mx_decode(uint32_t c, int e) {
  using X = MxF<F>;
  const float v = ldexpf(mx_value<F>(c & ((1u << (X::BITS - 1)) - 1u)), e - 127);
  return u2f(e == 255 ? kMxNaN : f2u(v) | ((c >> (X::BITS - 1)) << 31));
}

// 24-bit uniforms of the quad starting at element i: uniform01x4 (common.h) before its conversion
__device__ __forceinline__ void mx_rand24x4(uint64_t seed, uint64_t i, uint32_t* k) {
  uint32_t h = rand32(seed, i);
  k[0] = h >> 8;
  h = h ? h : 0x9E3779B9u;
#pragma unroll
  for (int j = 1; j < 4; ++j) {
    h ^= h << 13;
    h ^= h >> 17;
    h ^= h << 5;
    k[j] = h >> 8;
  }
}

// v (its bits above the field's width clear) into the little-endian bit stream d at bit `pos`
template <int N>
__device__ __forceinline__ void put_bits(uint32_t (&d)[N], int pos, uint32_t v) {
  d[pos >> 5] |= v << (pos & 31);
  if ((pos & 31) != 0 && (pos >> 5) + 1 < N) d[(pos >> 5) + 1] |= v >> ((32 - (pos & 31)) & 31);
}
template <int N>
__device__ __forceinline__ uint32_t get_bits(const uint32_t (&d)[N], int pos, int width) {
  uint32_t v = d[pos >> 5] >> (pos & 31);
  if ((pos & 31) + width > 32) v |= d[(pos >> 5) + 1] << ((32 - (pos & 31)) & 31);
  return v & ((1u << width) - 1u);
}

// a[i] for a lane-dependent i below T, by selects (a stays in registers)
template <int T, int W>
__device__ __forceinline__ void pick(const uint32_t (&a)[T][W], int i, uint32_t (&o)[W]) {
#pragma unroll
  for (int w = 0; w < W; ++w) {
    if constexpr (T == 2) {
      o[w] = (i & 1) ? a[1][w] : a[0][w];
    } else {
      const uint32_t lo = (i & 1) ? a[1][w] : a[0][w], hi = (i & 1) ? a[3][w] : a[2][w];
      o[w] = (i & 2) ? hi : lo;
    }
  }
}
template <int K>
__device__ __forceinline__ uint32_t quad_xor(uint32_t v) {
  static_assert(K >= 1 && K <= 3, "inside a quad");
  return dpp_u32<K == 1 ? 0xB1 : K == 2 ? 0x4E : 0x1B>(v);   // quad_perm [1,0,3,2] [2,3,0,1] [3,2,1,0]
}

constexpr int mx_gcd(int a, int b) { return b ? mx_gcd(b, a % b) : a; }

// ------------------------------------------------------------------------------------------------
// encode / fused world-1 step
template <typename E, int F, bool SR, bool FUSED>
__global__ __launch_bounds__(kMxBlock) void mx_encode_e(const E* __restrict__ x, int64_t n, uint64_t seed,
                                                        const float* __restrict__ u, uint8_t* __restrict__ payload,
                                                        E* __restrict__ out, int x16, int o16, int u16) {
  using X = MxF<F>;
  constexpr int G = MxE<E>::G, kRow = kWave * G, ROWS = kMxChunk / kRow;
  constexpr int LPB = 32 / G, BPR = kWave / LPB;            // lanes per block, blocks per row
  constexpr int I = X::BITS * G, W = (I + 31) / 32;         // a lane's codes of one row: bits, dwords
  constexpr int T = 32 / mx_gcd(I, 32), ND = T * I / 32;    // lanes (= rows) transposed; dwords stored
  constexpr int kRowBytes = kWave * I / 8, kChunkBytes = ROWS * kRowBytes;
  static_assert(ROWS % T == 0 && T <= 4 && BPR % 4 == 0 && ROWS * BPR == 32, "the chunk's split");

  const int lane = threadIdx.x & 63;
  const int64_t nb = (n + 31) >> 5;
  const int64_t sbytes = (nb + 15) & ~(int64_t)15;
  uint8_t* const codes = payload + sbytes;
  if constexpr (!FUSED) {
    if (blockIdx.x == 0 && threadIdx.x < 16) {              // the zero padding of both parts
      const int64_t cb = nb * 4 * X::BITS;
      if (nb + threadIdx.x < sbytes) payload[nb + threadIdx.x] = 0;
      if (cb + threadIdx.x < ((cb + 15) & ~(int64_t)15)) codes[cb + threadIdx.x] = 0;
    }
  }

  const int64_t nchunks = (n + kMxChunk - 1) / kMxChunk;
  const int64_t nwaves = (int64_t)gridDim.x * kMxWaves;
  int64_t c = (int64_t)blockIdx.x * kMxWaves + (threadIdx.x >> 6);
  u32x4 cur[ROWS], nxt[ROWS];
#pragma unroll
  for (int r = 0; r < ROWS; ++r) { cur[r] = (u32x4)(0u); nxt[r] = (u32x4)(0u); }
  if (c < nchunks) {
    const bool fast = x16 && (c + 1) * kMxChunk <= n;
#pragma unroll
    for (int r = 0; r < ROWS; ++r) cur[r] = mx_load<E>(x, c * kMxChunk + r * kRow + lane * G, n, fast);
  }
  for (; c < nchunks; c += nwaves) {
    const int64_t c2 = c + nwaves;
    if (c2 < nchunks) {   // the next chunk's loads fly over this chunk's conversion and stores
      const bool fast2 = x16 && (c2 + 1) * kMxChunk <= n;
#pragma unroll
      for (int r = 0; r < ROWS; ++r) nxt[r] = mx_load<E>(x, c2 * kMxChunk + r * kRow + lane * G, n, fast2);
    }
    const bool full = (c + 1) * kMxChunk <= n;   // the same in every lane of the wave
    uint32_t sc[8] = {0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u};      // the chunk's 32 scale bytes, wave-uniform
#pragma unroll
    for (int g = 0; g < ROWS / T; ++g) {
      uint32_t item[T][W];
#pragma unroll
      for (int q = 0; q < T; ++q) {
        const int row = g * T + q;
        const int64_t e0 = c * kMxChunk + row * kRow + lane * G;
        uint32_t v[G];
        MxE<E>::unpack(cur[row], v);
        uint32_t a = 0;
#pragma unroll
        for (int j = 0; j < G; ++j) a = max(a, v[j] & 0x7FFFFFFFu);
        a = LPB == 8 ? row8_max(a) : quad_max(a);
        const bool nanb = a >= 0x7F800000u;
        const int e = nanb ? 255 : min(max((int)(a >> 23) - X::EMAX, 0), 254);
        uint32_t k[G];
        if constexpr (SR) {
          if (u) {
#pragma unroll
            for (int h = 0; h < G / 4; ++h) {
              const u32x4 t = mx_load<float>(u, e0 + 4 * h, n, u16 && full);
#pragma unroll
              for (int j = 0; j < 4; ++j) k[4 * h + j] = (uint32_t)fminf(fmaxf(u2f(t[j]) * 16777216.0f, 0.0f), 16777215.0f);
            }
          } else {
#pragma unroll
            for (int h = 0; h < G / 4; ++h) mx_rand24x4(seed, (uint64_t)(e0 + 4 * h), k + 4 * h);
          }
        } else {
#pragma unroll
          for (int j = 0; j < G; ++j) k[j] = 0u;
        }
        if constexpr (FUSED) {
          float d[G];
#pragma unroll
          for (int j = 0; j < G; ++j) d[j] = mx_decode<F>(mx_code<F, SR>(v[j], e, k[j]), e);
          MxE<E>::put(out, e0, n, o16 && full, d);
        } else {
#pragma unroll
          for (int w = 0; w < W; ++w) item[q][w] = 0u;
#pragma unroll
          for (int j = 0; j < G; ++j) put_bits(item[q], j * X::BITS, nanb ? 0u : mx_code<F, SR>(v[j], e, k[j]));
          if (full) {
#pragma unroll
            for (int b = 0; b < BPR; ++b)
              sc[(row * BPR + b) >> 2] |= (uint32_t)__builtin_amdgcn_readlane(e, b * LPB) << (8 * (b & 3));
          } else {
            const int64_t blk = c * 32 + row * BPR + lane / LPB;
            if (blk < nb) {   // whole blocks: the positions past n are +0 and their codes 0
              if (lane % LPB == 0) payload[blk] = (uint8_t)e;
              uint8_t* p = codes + c * kChunkBytes + row * kRowBytes + lane * (I / 8);
#pragma unroll
              for (int t = 0; t < I / 8; ++t) p[t] = (uint8_t)(item[q][t >> 2] >> (8 * (t & 3)));
            }
          }
        }
      }
      if constexpr (!FUSED) {
        if (full) {
          // lane q of each group of T lanes gathers row q's items of the group, in lane order
          const int q = lane & (T - 1);
          uint32_t d[ND];
          if constexpr (T == 1) {
#pragma unroll
            for (int w = 0; w < W; ++w) d[w] = item[0][w];
          } else {
            uint32_t got[T][W], send[W];
            pick<T, W>(item, q, got[0]);          // lane q ^ k wants row q ^ k of this lane
            pick<T, W>(item, q ^ 1, send);
#pragma unroll
            for (int w = 0; w < W; ++w) got[1][w] = quad_xor<1>(send[w]);
            if constexpr (T == 4) {
              pick<T, W>(item, q ^ 2, send);
#pragma unroll
              for (int w = 0; w < W; ++w) got[2][w] = quad_xor<2>(send[w]);
              pick<T, W>(item, q ^ 3, send);
#pragma unroll
              for (int w = 0; w < W; ++w) got[3][w] = quad_xor<3>(send[w]);
            }
#pragma unroll
            for (int w = 0; w < ND; ++w) d[w] = 0u;
#pragma unroll
            for (int j = 0; j < T; ++j) {     // got[j ^ q] came from lane j of the group
              uint32_t piece[W];
              pick<T, W>(got, j ^ q, piece);
#pragma unroll
              for (int w = 0; w < W; ++w) put_bits(d, j * I + 32 * w, piece[w]);
            }
          }
          uint8_t* p = codes + c * kChunkBytes + (g * T + q) * kRowBytes + (lane / T) * (ND * 4);
          if constexpr (ND == 1) {
            __builtin_nontemporal_store(d[0], reinterpret_cast<uint32_t*>(p));
          } else if constexpr (ND == 2) {
            u32x2 t;
            t[0] = d[0]; t[1] = d[1];
            __builtin_nontemporal_store(t, reinterpret_cast<u32x2*>(p));
          } else {
            u32x3v t;
            t[0] = d[0]; t[1] = d[1]; t[2] = d[2];
            *reinterpret_cast<u32x3*>(p) = t;
          }
        }
      }
    }
    if constexpr (!FUSED) {
      if (full && lane == 0) {
        u32x4 s0, s1;
#pragma unroll
        for (int j = 0; j < 4; ++j) { s0[j] = sc[j]; s1[j] = sc[4 + j]; }
        u32x4* p = reinterpret_cast<u32x4*>(payload + c * 32);
        p[0] = s0;
        p[1] = s1;
      }
    }
#pragma unroll
    for (int r = 0; r < ROWS; ++r) cur[r] = nxt[r];
  }
}

// ------------------------------------------------------------------------------------------------
// decode + aggregate: W rank-major payloads, summed in rank order, one division, one rounding
template <typename O, int F>
__global__ __launch_bounds__(kMxBlock) void mx_decode_e(const uint8_t* __restrict__ payloads, int64_t stride, int world,
                                                        int64_t n, float divisor, O* __restrict__ out, int o16) {
  using X = MxF<F>;
  constexpr int NL = X::BITS == 6 ? 3 : 1;          // 16-B lines of codes a thread decodes
  constexpr int NE = NL * 128 / X::BITS;            // their elements: 16, 64 or 32
  constexpr int NS = NE > 32 ? NE / 32 : 1;         // their scale bytes
  constexpr int G = MxE<O>::G;
  const int64_t nb = (n + 31) >> 5;
  const int64_t sbytes = (nb + 15) & ~(int64_t)15;
  const int64_t lines = (nb * 4 * X::BITS + 15) >> 4;
  const int64_t ng = (n + NE - 1) / NE;
  for (int64_t g = (int64_t)blockIdx.x * kMxBlock + threadIdx.x; g < ng; g += (int64_t)gridDim.x * kMxBlock) {
    const int64_t e0 = g * NE, blk = e0 >> 5;
    float acc[NE];
    for (int w = 0; w < world; ++w) {
      const uint8_t* p = payloads + w * stride;
      int e[NS];
#pragma unroll
      for (int s = 0; s < NS; ++s) e[s] = blk + s < nb ? (int)p[blk + s] : 0;
      uint32_t wd[4 * NL];
#pragma unroll
      for (int l = 0; l < NL; ++l) {
        const int64_t line = g * NL + l;
        const u32x4 t = line < lines ? *reinterpret_cast<const u32x4*>(p + sbytes + 16 * line) : (u32x4)(0u);
#pragma unroll
        for (int j = 0; j < 4; ++j) wd[4 * l + j] = t[j];
      }
#pragma unroll
      for (int j = 0; j < NE; ++j) {
        const float d = mx_decode<F>(get_bits(wd, j * X::BITS, X::BITS), e[j >> 5]);
        acc[j] = w == 0 ? d : acc[j] + d;
      }
    }
    const bool fast = o16 && e0 + NE <= n;
#pragma unroll
    for (int h = 0; h < NE / G; ++h) {
      float d[G];
#pragma unroll
      for (int j = 0; j < G; ++j) d[j] = divisor == 1.0f ? acc[h * G + j] : acc[h * G + j] / divisor;
      MxE<O>::put(out, e0 + h * G, n, fast, d);
    }
  }
}

// ------------------------------------------------------------------------------------------------
// host side: one typed launcher per f32 / bf16 pair
template <typename E, int F, bool FUSED>
static void mx_launch(unsigned grid, hipStream_t st, int sr, const E* x, int64_t n, uint64_t seed, const float* u,
                      uint8_t* payload, E* out) {
  const int x16 = al16(x), o16 = al16(out), u16 = al16(u);
  if (sr) mx_encode_e<E, F, true, FUSED><<<grid, kMxBlock, 0, st>>>(x, n, seed, u, payload, out, x16, o16, u16);
  else mx_encode_e<E, F, false, FUSED><<<grid, kMxBlock, 0, st>>>(x, n, seed, u, payload, out, x16, o16, u16);
}

template <typename E, bool FUSED>
static grace_status_t mx_encode(const char* name, const char* bad, const E* x, int64_t n, int32_t format,
                                int32_t rounding, uint64_t seed, const float* u, uint8_t* payload, E* out,
                                void* stream) {
  GRACE_REQUIRE(x && (FUSED ? out != nullptr : payload != nullptr) && n >= 0 && n <= INT32_MAX &&
                    mx_format_ok(format) && (rounding == 0 || rounding == 1) && MxE<E>::addressable(x) &&
                    MxE<E>::addressable(out) && al16(payload) && al4(u),
                bad);
  if (n == 0) return GRACE_OK;
  const hipStream_t st = as_stream(stream);
  const unsigned grid = stream_grid((n + kMxChunk - 1) / kMxChunk, kMxWaves, kMxGridCap);
  switch (format) {
    case 0: mx_launch<E, 0, FUSED>(grid, st, rounding, x, n, seed, u, payload, out); break;
    case 1: mx_launch<E, 1, FUSED>(grid, st, rounding, x, n, seed, u, payload, out); break;
    case 2: mx_launch<E, 2, FUSED>(grid, st, rounding, x, n, seed, u, payload, out); break;
    case 3: mx_launch<E, 3, FUSED>(grid, st, rounding, x, n, seed, u, payload, out); break;
    default: mx_launch<E, 4, FUSED>(grid, st, rounding, x, n, seed, u, payload, out); break;
  }
  GRACE_CHECK_LAUNCH(name);
  return GRACE_OK;
}

template <typename O, int F>
static void mx_launch_decode(hipStream_t st, const uint8_t* payloads, int64_t stride, int32_t world, int64_t n,
                             float divisor, O* out) {
  constexpr int NE = (MxF<F>::BITS == 6 ? 3 : 1) * 128 / MxF<F>::BITS;
  mx_decode_e<O, F><<<stream_grid((n + NE - 1) / NE, kMxBlock, kMxDecGridCap), kMxBlock, 0, st>>>(
      payloads, stride, world, n, divisor, out, al16(out) ? 1 : 0);
}

template <typename O>
static grace_status_t mx_decode_host(const char* name, const char* bad, const uint8_t* payloads, int64_t stride,
                                     int32_t world, int64_t n, int32_t format, float divisor, O* out, void* stream) {
  GRACE_REQUIRE(payloads && out && world >= 1 && world <= 1024 && n >= 0 && n <= INT32_MAX && mx_format_ok(format) &&
                    divisor != 0.0f && al16(payloads) && stride >= 0 && stride % 16 == 0 &&
                    (size_t)stride >= (n ? mx_bytes(n, format) : 0) && MxE<O>::addressable(out),
                bad);
  if (n == 0) return GRACE_OK;
  const hipStream_t st = as_stream(stream);
  switch (format) {
    case 0: mx_launch_decode<O, 0>(st, payloads, stride, world, n, divisor, out); break;
    case 1: mx_launch_decode<O, 1>(st, payloads, stride, world, n, divisor, out); break;
    case 2: mx_launch_decode<O, 2>(st, payloads, stride, world, n, divisor, out); break;
    case 3: mx_launch_decode<O, 3>(st, payloads, stride, world, n, divisor, out); break;
    default: mx_launch_decode<O, 4>(st, payloads, stride, world, n, divisor, out); break;
  }
  GRACE_CHECK_LAUNCH(name);
  return GRACE_OK;
}

}  // namespace grace

using namespace grace;

extern "C" {

size_t grace_mx_payload_bytes(int64_t n, int32_t format) {
  return n >= 1 && n <= INT32_MAX && mx_format_ok(format) ? mx_bytes(n, format) : 0;
}

grace_status_t grace_mx_compress(const float* x, int64_t n, int32_t format, int32_t rounding, uint64_t seed,
                                 const float* u, uint8_t* payload, void* stream) {
  return mx_encode<float, false>("grace_mx_compress", "grace_mx_compress: bad arguments", x, n, format, rounding, seed,
                                 u, payload, nullptr, stream);
}

grace_status_t grace_mx_compress_bf16(const uint16_t* x, int64_t n, int32_t format, int32_t rounding, uint64_t seed,
                                      const float* u, uint8_t* payload, void* stream) {
  return mx_encode<uint16_t, false>("grace_mx_compress_bf16", "grace_mx_compress_bf16: bad arguments", x, n, format,
                                    rounding, seed, u, payload, nullptr, stream);
}

grace_status_t grace_mx_step_w1(const float* x, int64_t n, int32_t format, int32_t rounding, uint64_t seed,
                                const float* u, float* out, void* stream) {
  return mx_encode<float, true>("grace_mx_step_w1", "grace_mx_step_w1: bad arguments", x, n, format, rounding, seed, u,
                                nullptr, out, stream);
}

grace_status_t grace_mx_step_w1_bf16(const uint16_t* x, int64_t n, int32_t format, int32_t rounding, uint64_t seed,
                                     const float* u, uint16_t* out, void* stream) {
  return mx_encode<uint16_t, true>("grace_mx_step_w1_bf16", "grace_mx_step_w1_bf16: bad arguments", x, n, format,
                                   rounding, seed, u, nullptr, out, stream);
}

grace_status_t grace_mx_decode_aggregate(const uint8_t* payloads, int64_t stride_bytes, int32_t world, int64_t n,
                                         int32_t format, float divisor, float* out, void* stream) {
  return mx_decode_host<float>("grace_mx_decode_aggregate", "grace_mx_decode_aggregate: bad arguments", payloads,
                               stride_bytes, world, n, format, divisor, out, stream);
}

grace_status_t grace_mx_decode_aggregate_bf16(const uint8_t* payloads, int64_t stride_bytes, int32_t world, int64_t n,
                                              int32_t format, float divisor, uint16_t* out, void* stream) {
  return mx_decode_host<uint16_t>("grace_mx_decode_aggregate_bf16", "grace_mx_decode_aggregate_bf16: bad arguments",
                                  payloads, stride_bytes, world, n, format, divisor, out, stream);
}

}  // extern "C"
