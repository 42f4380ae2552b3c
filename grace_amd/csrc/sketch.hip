// Quantile-bucket quantisation (SketchML): exact multi-select, search + sums + pack,
// and a one-launch W-rank decode.
//
// The multi-select finds all q + 1 order statistics together by radix refinement over the
// order-preserving 32-bit key, digits of 14 / 6 / 6 / 6 bits from the top: four passes over an f32 x
// whatever the data, two over a bf16 x (its keys have 16 significant bits; 14 + 6 covers them).
//   pass 0   every element counts in a 16384-bin LDS histogram (64 KB) of its top digit;
//   pass L   an element whose higher digits are one of the live prefixes -- the at most q + 1
//            prefixes some rank is still inside, sorted, found by a branch-free search of the table
//            in LDS -- counts in that prefix's 64-bin histogram (257 x 64 x 4 B = 64.25 KB of LDS);
//   flush    the workgroup's non-zero bins go to the global histogram with integer atomics;
//   resolve  one workgroup between passes walks the counts for every rank at once: a block scan over
//            the top-digit histogram, then one wave per rank over its prefix's 64 bins; ranks are
//            ascending, so equal new prefixes are neighbours and one scan builds the next table.
// Counts are integers, so the edges are exact and the same on every call.
//
// The encode pass stages the q - 1 interior edges in LDS, padded with NaN (which compares false) to
// 15 or 255 entries, searches them branch-free in 4 or 8 steps, packs a lane's 4 or 8 codes into one
// store and adds the element to its bucket's f64 sum and count in LDS (16 lane-selected copies of
// the table when q <= 16, against contention); the workgroup's partials are combined in the
// workspace with atomics and a last small kernel divides.
//
// The world-1 step keeps the packed codes in the workspace and decodes them with the W-rank kernel.
//
// Operands off their vector grid, and the group that crosses n, go through guarded per-element
// accesses in the same kernels: nothing outside [0, n) (or the ceil(n / 2) packed bytes) is touched.
#include "select.h"

#include "../../include/grace_hip_sketch.h"

namespace grace {

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));

constexpr int kSkSelBlock = 1024;              // select passes and resolve: 16 waves
constexpr int kSkSelWaves = kSkSelBlock / kWave;
constexpr int kSkSelGridCap = 512;             // two 64-KB workgroups a CU; one sweep = 2^21 f32 / 2^22 bf16 elements
constexpr int kSkBlock = 256;                  // encode and decode
constexpr int kSkGridCap = 2048;               // one sweep = 2^21 f32 / 2^22 bf16 elements
constexpr int kSkTopBits = 14, kSkTopBins = 1 << kSkTopBits;
constexpr int kSkDigBits = 6, kSkDigBins = 1 << kSkDigBits;
constexpr int kSkRanks = 257;                  // q + 1 at most: live prefixes at most
constexpr int kSkPrefPad = 512;                // the table is searched as 2^k - 1 <= 511 entries
constexpr int kSkBuckets = 256;
constexpr uint32_t kSkNoPrefix = 0xFFFFFFFFu;  // above every prefix (a prefix has at most 26 bits)
constexpr int kSkStageMax = 16384;             // decode: world * q means at most staged in LDS (64 KB)

// workspace layout, in bytes
constexpr size_t kSkLevelBytes = sizeof(uint32_t) * kSkRanks * kSkDigBins;
constexpr size_t kSkOffTop = 0;                                                 // u32[16384]
constexpr size_t kSkOffLevel = kSkOffTop + sizeof(uint32_t) * kSkTopBins;       // 3 x u32[257 * 64]
constexpr size_t kSkOffSum = kSkOffLevel + 3 * kSkLevelBytes;                   // f64[256]
constexpr size_t kSkOffCnt = kSkOffSum + sizeof(double) * kSkBuckets;           // u32[256]
constexpr size_t kSkOffState = kSkOffCnt + sizeof(uint32_t) * kSkBuckets;       // everything before is zeroed per call
constexpr int kStLive = 0, kStPref = 4, kStSlot = kStPref + kSkPrefPad, kStRem = kStSlot + 264, kStWords = kStRem + 264;
constexpr size_t kSkOffEdges = kSkOffState + sizeof(uint32_t) * kStWords;       // f32[257]
constexpr size_t kSkOffCodes = (kSkOffEdges + sizeof(float) * 260 + 255) & ~(size_t)255;
static_assert(kSkOffSum % 8 == 0 && kSkOffState % 4 == 0, "f64 sums on their grid");

// Order-preserving key: ascending keys are ascending f32 values; a zero of either sign is +0.0.
__device__ __forceinline__ uint32_t order_key(float x) {
  uint32_t u = f2u(x);
  u = u == 0x80000000u ? 0u : u;
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float key_value(uint32_t k) { return u2f((k & 0x80000000u) ? (k ^ 0x80000000u) : ~k); }

// ------------------------------------------------------------------------------------------------
// element access: G elements are 16 B of the gradient or the dense result
template <typename E>
struct SkE;

template <>
struct SkE<float> {
  static constexpr int G = 4;
  static bool addressable(const void* p) { return al4(p); }
  static __device__ __forceinline__ float ld(const float* p, int64_t i) { return p[i]; }
  static __device__ __forceinline__ void st(float* p, int64_t i, float v) { p[i] = v; }
  static __device__ __forceinline__ void unpack(u32x4 t, float (&v)[4]) {
    v[0] = u2f(t[0]); v[1] = u2f(t[1]); v[2] = u2f(t[2]); v[3] = u2f(t[3]);
  }
  static __device__ __forceinline__ u32x4 pack(const float (&d)[4]) {
    u32x4 t;
#pragma unroll
    for (int j = 0; j < 4; ++j) t[j] = f2u(d[j]);
    return t;
  }
};

template <>
struct SkE<uint16_t> {
  static constexpr int G = 8;
  static bool addressable(const void* p) { return al2(p); }
  static __device__ __forceinline__ float ld(const uint16_t* p, int64_t i) { return bf16_to_f32(p[i]); }
  static __device__ __forceinline__ void st(uint16_t* p, int64_t i, float v) { p[i] = f32_to_bf16(v); }
  static __device__ __forceinline__ void unpack(u32x4 t, float (&v)[8]) {
#pragma unroll
    for (int k = 0; k < 4; ++k) { v[2 * k] = u2f(t[k] << 16); v[2 * k + 1] = u2f(t[k] & 0xFFFF0000u); }
  }
  static __device__ __forceinline__ u32x4 pack(const float (&d)[8]) {
    u32x4 t;
#pragma unroll
    for (int k = 0; k < 4; ++k) t[k] = pack_bf16x2(d[2 * k], d[2 * k + 1]);
    return t;
  }
};

// v[j] = x[e + j]; 0 where e + j >= n (the caller counts only j with fast || e + j < n)
template <typename E>
__device__ __forceinline__ void load_vals(const E* x, int64_t e, int64_t n, bool fast, float (&v)[SkE<E>::G]) {
  if (fast) {
    SkE<E>::unpack(*reinterpret_cast<const u32x4*>(x + e), v);
  } else {
#pragma unroll
    for (int j = 0; j < SkE<E>::G; ++j) v[j] = e + j < n ? SkE<E>::ld(x, e + j) : 0.f;
  }
}

template <typename E>
__device__ __forceinline__ void store_vals(E* o, int64_t e, int64_t n, bool fast, const float (&d)[SkE<E>::G]) {
  if (fast) {
    __builtin_nontemporal_store(SkE<E>::pack(d), reinterpret_cast<u32x4*>(o + e));
  } else {
#pragma unroll
    for (int j = 0; j < SkE<E>::G; ++j)
      if (e + j < n) SkE<E>::st(o, e + j, d[j]);
  }
}

// The codes of the group at element e (a multiple of G, so even): one byte each, or two to a byte
// with element 2i in the low nibble.  c[j] is 0 where e + j >= n.
template <int G, bool NIB>
__device__ __forceinline__ void store_codes(uint8_t* c, int64_t e, int64_t n, bool fast, const uint32_t (&b)[G]) {
  if constexpr (NIB) {
    uint32_t w = 0;
#pragma unroll
    for (int j = 0; j < G; ++j) w |= b[j] << (4 * j);
    if (fast) {
      if constexpr (G == 4) *reinterpret_cast<uint16_t*>(c + (e >> 1)) = (uint16_t)w;
      else *reinterpret_cast<uint32_t*>(c + (e >> 1)) = w;
    } else {
#pragma unroll
      for (int k = 0; k < G / 2; ++k)
        if (e + 2 * k < n) c[(e >> 1) + k] = (uint8_t)(w >> (8 * k));
    }
  } else {
    if (fast) {
      uint32_t w[G / 4];
#pragma unroll
      for (int k = 0; k < G / 4; ++k)
        w[k] = b[4 * k] | (b[4 * k + 1] << 8) | (b[4 * k + 2] << 16) | (b[4 * k + 3] << 24);
      if constexpr (G == 4) {
        *reinterpret_cast<uint32_t*>(c + e) = w[0];
      } else {
        u32x2 t;
        t[0] = w[0]; t[1] = w[1];
        *reinterpret_cast<u32x2*>(c + e) = t;
      }
    } else {
#pragma unroll
      for (int j = 0; j < G; ++j)
        if (e + j < n) c[e + j] = (uint8_t)b[j];
    }
  }
}

template <int G, bool NIB>
__device__ __forceinline__ void load_codes(const uint8_t* c, int64_t e, int64_t n, bool fast, uint32_t (&b)[G]) {
  if constexpr (NIB) {
    uint32_t w = 0;
    if (fast) {
      if constexpr (G == 4) w = *reinterpret_cast<const uint16_t*>(c + (e >> 1));
      else w = *reinterpret_cast<const uint32_t*>(c + (e >> 1));
    } else {
#pragma unroll
      for (int k = 0; k < G / 2; ++k)
        if (e + 2 * k < n) w |= (uint32_t)c[(e >> 1) + k] << (8 * k);
    }
#pragma unroll
    for (int j = 0; j < G; ++j) b[j] = (w >> (4 * j)) & 15u;
  } else {
    if (fast) {
      uint32_t w[G / 4];
      if constexpr (G == 4) {
        w[0] = *reinterpret_cast<const uint32_t*>(c + e);
      } else {
        const u32x2 t = *reinterpret_cast<const u32x2*>(c + e);
        w[0] = t[0]; w[1] = t[1];
      }
#pragma unroll
      for (int j = 0; j < G; ++j) b[j] = (w[j >> 2] >> (8 * (j & 3))) & 255u;
    } else {
#pragma unroll
      for (int j = 0; j < G; ++j) b[j] = e + j < n ? (uint32_t)c[e + j] : 0u;
    }
  }
}

// ------------------------------------------------------------------------------------------------
// multi-select
__global__ __launch_bounds__(kSkSelBlock) void sk_zero(uint32_t* __restrict__ p, int words) {
  for (int i = blockIdx.x * kSkSelBlock + threadIdx.x; i < words; i += gridDim.x * kSkSelBlock) p[i] = 0u;
}

// One histogram pass.  TOP: the top 14 bits of every key.  Otherwise `shift` key bits lie below the
// prefix, the digit is the 6 bits under it, and only keys whose prefix is live count.
template <typename E, bool TOP>
__global__ __launch_bounds__(kSkSelBlock) void sk_hist_e(const E* __restrict__ x, int64_t n, int shift,
                                                         const uint32_t* __restrict__ state,
                                                         uint32_t* __restrict__ hist, int aligned) {
  constexpr int G = SkE<E>::G;
  __shared__ uint32_t sh_h[TOP ? kSkTopBins : kSkRanks * kSkDigBins];
  __shared__ uint32_t sh_p[TOP ? 1 : kSkPrefPad];
  int nbins = kSkTopBins, top = 0;
  if constexpr (!TOP) {
    const int nlive = min((int)state[kStLive], kSkRanks);
    for (int i = threadIdx.x; i < kSkPrefPad; i += kSkSelBlock) sh_p[i] = state[kStPref + i];
    top = 1;
    while (2 * top - 1 < nlive) top <<= 1;       // the sorted table, padded above, as 2 top - 1 entries
    nbins = nlive * kSkDigBins;
  }
  for (int b = threadIdx.x; b < nbins; b += kSkSelBlock) sh_h[b] = 0u;
  __syncthreads();

  const int64_t ng = (n + G - 1) / G;
#pragma unroll 2
  for (int64_t g = (int64_t)blockIdx.x * kSkSelBlock + threadIdx.x; g < ng; g += (int64_t)gridDim.x * kSkSelBlock) {
    const int64_t e = g * G;
    const bool fast = aligned && e + G <= n;
    float v[G];
    load_vals<E>(x, e, n, fast, v);
    if constexpr (TOP) {
#pragma unroll
      for (int j = 0; j < G; ++j)
        if (fast || e + j < n) atomicAdd(&sh_h[order_key(v[j]) >> (32 - kSkTopBits)], 1u);
    } else {
      uint32_t k[G], p[G];
      int pos[G];
#pragma unroll
      for (int j = 0; j < G; ++j) { k[j] = order_key(v[j]); p[j] = k[j] >> shift; pos[j] = 0; }
      for (int s = top; s > 0; s >>= 1) {        // pos = #{i : prefix[i] <= p}, the G searches in step
        uint32_t t[G];
#pragma unroll
        for (int j = 0; j < G; ++j) t[j] = sh_p[pos[j] + s - 1];
#pragma unroll
        for (int j = 0; j < G; ++j) pos[j] += t[j] <= p[j] ? s : 0;
      }
#pragma unroll
      for (int j = 0; j < G; ++j)
        if ((fast || e + j < n) && pos[j] > 0 && sh_p[pos[j] - 1] == p[j])
          atomicAdd(&sh_h[(pos[j] - 1) * kSkDigBins + ((k[j] >> (shift - kSkDigBits)) & (kSkDigBins - 1))], 1u);
    }
  }
  __syncthreads();
  for (int b = threadIdx.x; b < nbins; b += kSkSelBlock) {
    const uint32_t c = sh_h[b];
    if (c) atomicAdd(hist + b, c);
  }
}

// Between passes, one workgroup: for every rank j the bin its remaining rank falls in, the rank
// inside that bin, and the sorted table of the distinct new prefixes.  After the last pass the
// prefixes are whole keys (bf16: the top 20 bits of one, `lowbits` = 12 below) and become the edges.
template <bool TOP>
__global__ __launch_bounds__(kSkSelBlock) void sk_resolve(const uint32_t* __restrict__ hist, uint32_t* __restrict__ state,
                                                          int64_t n, int q, int last, int lowbits,
                                                          float* __restrict__ edges) {
  __shared__ uint32_t s_w[kSkSelWaves + 1];
  __shared__ uint32_t s_rank[kSkRanks], s_slot[kSkRanks], s_pref[kSkRanks], s_new[kSkRanks], s_rem[kSkRanks];
  const int t = threadIdx.x, nr = q + 1;
  if constexpr (TOP) {
    if (t < nr) s_rank[t] = (uint32_t)(((int64_t)t * (n - 1)) / q);
    constexpr int PER = kSkTopBins / kSkSelBlock;
    uint32_t h[PER], s = 0;
#pragma unroll
    for (int j = 0; j < PER; ++j) { h[j] = hist[t * PER + j]; s += h[j]; }
    const uint32_t ex = block_excl_scan<kSkSelBlock>(s, s_w, nullptr);   // its barriers publish s_rank
    for (int j = 0; j < nr; ++j) {
      const uint32_t r = s_rank[j];
      if (ex <= r && r - ex < s) {               // the counts sum to n > r: one thread owns each rank
        uint32_t acc = ex;
        int d = PER - 1;
        bool found = false;
#pragma unroll
        for (int i = 0; i < PER; ++i) {
          if (!found && r - acc < h[i]) { d = i; found = true; }
          if (!found) acc += h[i];
        }
        s_new[j] = (uint32_t)(t * PER + d);
        s_rem[j] = r - acc;
      }
    }
  } else {
    if (t < nr) {
      s_rank[t] = state[kStRem + t];
      s_slot[t] = min(state[kStSlot + t], (uint32_t)(kSkRanks - 1));
    }
    if (t < kSkRanks) s_pref[t] = state[kStPref + t];
    __syncthreads();
    const int lane = t & 63;
    for (int j = t >> 6; j < nr; j += kSkSelWaves) {   // a wave per rank: scan the 64 bins of its prefix
      const uint32_t slot = s_slot[j], r = s_rank[j];
      const uint32_t c = hist[slot * kSkDigBins + lane];
      uint32_t inc = c;
#pragma unroll
      for (int o = 1; o < 64; o <<= 1) {
        const uint32_t u = __shfl_up(inc, o, 64);
        if (lane >= o) inc += u;
      }
      const uint32_t exc = inc - c;
      const uint64_t hit = __ballot(exc <= r && r < inc);
      const int d = hit ? __builtin_ctzll(hit) : kSkDigBins - 1;
      const uint32_t below = __shfl(exc, d, 64);
      if (lane == 0) {
        s_new[j] = (s_pref[slot] << kSkDigBits) | (uint32_t)d;
        s_rem[j] = hit ? r - below : 0u;
      }
    }
  }
  __syncthreads();
  if (last) {
    if (t < nr) {
      // the bits below a bf16 key's 16 are the sign's complement image: zeros for x >= 0, ones for x < 0
      const uint32_t k = s_new[t] << lowbits;
      edges[t] = key_value((k & 0x80000000u) ? k : k | ((1u << lowbits) - 1u));
    }
    return;
  }
  // ranks ascend, so do their prefixes: the distinct ones, in order, are the next table
  const uint32_t first = t < nr && (t == 0 || s_new[t] != s_new[t - 1]) ? 1u : 0u;
  uint32_t live;
  const uint32_t at = block_excl_scan<kSkSelBlock>(first, s_w, &live);
  if (t < nr) {
    state[kStSlot + t] = at + first - 1u;
    state[kStRem + t] = s_rem[t];
    if (first) state[kStPref + at] = s_new[t];
  }
  if (t < kSkPrefPad && t >= (int)live) state[kStPref + t] = kSkNoPrefix;
  if (t == 0) state[kStLive] = live;
}

// ------------------------------------------------------------------------------------------------
// search + sums + pack
template <typename E, bool NIB>
__global__ __launch_bounds__(kSkBlock) void sk_encode_e(const E* __restrict__ x, int64_t n, int q,
                                                        const float* __restrict__ edges, uint8_t* __restrict__ codes,
                                                        double* __restrict__ gsum, uint32_t* __restrict__ gcnt,
                                                        int aligned) {
  constexpr int G = SkE<E>::G;
  constexpr int T = NIB ? 16 : 256;              // T - 1 table entries, log2(T) steps
  __shared__ float sh_e[T];
  __shared__ double sh_s[kSkBuckets];
  __shared__ uint32_t sh_c[kSkBuckets];
  static_assert(kSkBlock == kSkBuckets && T <= kSkBlock, "one thread per table entry");
  if (threadIdx.x < T) sh_e[threadIdx.x] = (int)threadIdx.x < q - 1 ? edges[threadIdx.x + 1] : __builtin_nanf("");
  sh_s[threadIdx.x] = 0.0;
  sh_c[threadIdx.x] = 0u;
  __syncthreads();
  const uint32_t copy = NIB ? (threadIdx.x & 15u) << 4 : 0u;   // q <= 16: 16 copies of the 16 buckets

  const int64_t ng = (n + G - 1) / G;
#pragma unroll 2
  for (int64_t g = (int64_t)blockIdx.x * kSkBlock + threadIdx.x; g < ng; g += (int64_t)gridDim.x * kSkBlock) {
    const int64_t e = g * G;
    const bool fast = aligned && e + G <= n;
    float v[G];
    uint32_t pos[G];
    load_vals<E>(x, e, n, fast, v);
#pragma unroll
    for (int j = 0; j < G; ++j) pos[j] = 0u;
#pragma unroll
    for (int s = T / 2; s > 0; s >>= 1) {        // pos = #{i : edges[i + 1] <= v}; -0 == +0, NaN counts nothing
      float ed[G];
#pragma unroll
      for (int j = 0; j < G; ++j) ed[j] = sh_e[pos[j] + s - 1];
#pragma unroll
      for (int j = 0; j < G; ++j) pos[j] += ed[j] <= v[j] ? (uint32_t)s : 0u;
    }
#pragma unroll
    for (int j = 0; j < G; ++j) {
      if (fast || e + j < n) {
        atomicAdd(&sh_s[copy + pos[j]], (double)v[j]);
        atomicAdd(&sh_c[copy + pos[j]], 1u);
      } else {
        pos[j] = 0u;
      }
    }
    store_codes<G, NIB>(codes, e, n, fast, pos);
  }
  __syncthreads();
  // one partial a bucket and workgroup goes to the workspace: the 16 copies are summed here first
  double s = sh_s[threadIdx.x];
  uint32_t c = sh_c[threadIdx.x];
  if constexpr (NIB) {
    if (threadIdx.x >= 16) return;
#pragma unroll
    for (int k = 1; k < 16; ++k) { s += sh_s[16 * k + threadIdx.x]; c += sh_c[16 * k + threadIdx.x]; }
  }
  if (c) {
    unsafeAtomicAdd(gsum + threadIdx.x, s);
    atomicAdd(gcnt + threadIdx.x, c);
  }
}

__global__ __launch_bounds__(kSkBlock) void sk_means(const double* __restrict__ gsum, const uint32_t* __restrict__ gcnt,
                                                     int q, float* __restrict__ means) {
  const int b = threadIdx.x;
  if (b < q) means[b] = gcnt[b] ? (float)(gsum[b] / (double)gcnt[b]) : 0.f;
}

// ------------------------------------------------------------------------------------------------
// decode + aggregate: W rank-major payloads, summed in rank order, one division, one rounding.
// STAGED: all world * q means sit in LDS (world * q <= kSkStageMax); otherwise they are read from
// global memory, where the q-entry rows of the ranks being summed stay in cache.
template <typename O, bool NIB, bool STAGED>
__global__ __launch_bounds__(kSkBlock) void sk_decode_e(const uint8_t* __restrict__ codes, int64_t stride,
                                                        const float* __restrict__ means, int world, int64_t n, int q,
                                                        float divisor, O* __restrict__ out, int aligned) {
  constexpr int G = SkE<O>::G;
  extern __shared__ float sh_m[];
  if constexpr (STAGED) {
    for (int i = threadIdx.x; i < world * q; i += kSkBlock) sh_m[i] = means[i];
    __syncthreads();
  }
  const uint32_t top = (uint32_t)(q - 1);
  const int64_t ng = (n + G - 1) / G;
  for (int64_t g = (int64_t)blockIdx.x * kSkBlock + threadIdx.x; g < ng; g += (int64_t)gridDim.x * kSkBlock) {
    const int64_t e = g * G;
    const bool fast = aligned && e + G <= n;
    float acc[G];
#pragma unroll
    for (int j = 0; j < G; ++j) acc[j] = 0.f;
    for (int w = 0; w < world; ++w) {
      uint32_t cd[G];
      load_codes<G, NIB>(codes + w * stride, e, n, fast, cd);
#pragma unroll
      for (int j = 0; j < G; ++j) {
        const uint32_t i = (uint32_t)(w * q) + min(cd[j], top);
        acc[j] = acc[j] + (STAGED ? sh_m[i] : means[i]);
      }
    }
#pragma unroll
    for (int j = 0; j < G; ++j) acc[j] = divisor == 1.0f ? acc[j] : acc[j] / divisor;
    store_vals<O>(out, e, n, fast, acc);
  }
}

// ------------------------------------------------------------------------------------------------
// host side: one typed launcher per f32 / bf16 pair
static inline bool shape_ok(int64_t n, int32_t q) { return n >= 0 && n < ((int64_t)1 << 31) && q >= 2 && q <= 256; }
static inline int64_t code_bytes(int64_t n, int32_t q) { return q > 16 ? n : (n + 1) / 2; }

// The zeroing kernel and the passes and resolves of the select; the edges go to `edges` (q + 1 f32).
template <typename E>
static grace_status_t sk_select(const char* name, const E* x, int64_t n, int32_t q, float* edges, uint8_t* ws,
                                hipStream_t st) {
  constexpr int G = SkE<E>::G;
  constexpr int kLevels = sizeof(E) == 4 ? 4 : 2;     // bf16 keys: 16 significant bits, 14 + 6 covers them
  uint32_t* top = reinterpret_cast<uint32_t*>(ws + kSkOffTop);
  uint32_t* state = reinterpret_cast<uint32_t*>(ws + kSkOffState);
  const int al = al16(x) ? 1 : 0;
  const unsigned grid = stream_grid((n + G - 1) / G, kSkSelBlock, kSkSelGridCap);
  sk_zero<<<64, kSkSelBlock, 0, st>>>(top, (int)(kSkOffState / sizeof(uint32_t)));
  GRACE_CHECK_LAUNCH(name);
  sk_hist_e<E, true><<<grid, kSkSelBlock, 0, st>>>(x, n, 0, state, top, al);
  GRACE_CHECK_LAUNCH(name);
  sk_resolve<true><<<1, kSkSelBlock, 0, st>>>(top, state, n, q, 0, 0, edges);
  GRACE_CHECK_LAUNCH(name);
  for (int l = 1; l < kLevels; ++l) {
    uint32_t* hist = reinterpret_cast<uint32_t*>(ws + kSkOffLevel + (l - 1) * kSkLevelBytes);
    const int shift = 32 - kSkTopBits - kSkDigBits * (l - 1);
    sk_hist_e<E, false><<<grid, kSkSelBlock, 0, st>>>(x, n, shift, state, hist, al);
    GRACE_CHECK_LAUNCH(name);
    sk_resolve<false><<<1, kSkSelBlock, 0, st>>>(hist, state, n, q, l == kLevels - 1 ? 1 : 0, shift - kSkDigBits, edges);
    GRACE_CHECK_LAUNCH(name);
  }
  return GRACE_OK;
}

template <typename O>
static grace_status_t sk_launch_decode(const char* name, const uint8_t* codes, int64_t stride, const float* means,
                                       int32_t world, int64_t n, int32_t q, float divisor, O* out, hipStream_t st) {
  constexpr int G = SkE<O>::G;
  const int al = al8(codes) && (world == 1 || stride % 8 == 0) && al16(out);
  const bool staged = (int64_t)world * q <= kSkStageMax;
  const size_t lds = staged ? sizeof(float) * world * q : 0;
  const unsigned grid = stream_grid((n + G - 1) / G, kSkBlock, kSkGridCap);
  if (q <= 16) {
    if (staged) sk_decode_e<O, true, true><<<grid, kSkBlock, lds, st>>>(codes, stride, means, world, n, q, divisor, out, al);
    else sk_decode_e<O, true, false><<<grid, kSkBlock, 0, st>>>(codes, stride, means, world, n, q, divisor, out, al);
  } else {
    if (staged) sk_decode_e<O, false, true><<<grid, kSkBlock, lds, st>>>(codes, stride, means, world, n, q, divisor, out, al);
    else sk_decode_e<O, false, false><<<grid, kSkBlock, 0, st>>>(codes, stride, means, world, n, q, divisor, out, al);
  }
  GRACE_CHECK_LAUNCH(name);
  return GRACE_OK;
}

template <typename E>
static grace_status_t sk_edges(const char* name, const char* bad, const E* x, int64_t n, int32_t q, float* edges,
                               void* ws, void* stream) {
  GRACE_REQUIRE(x && edges && ws && shape_ok(n, q) && SkE<E>::addressable(x) && al4(edges) && al8(ws), bad);
  if (n == 0) return GRACE_OK;
  return sk_select<E>(name, x, n, q, edges, static_cast<uint8_t*>(ws), as_stream(stream));
}

// compress (out == nullptr) and the world-1 step (codes == nullptr: they live in the workspace)
template <typename E>
static grace_status_t sk_encode(const char* name, const char* bad, const E* x, int64_t n, int32_t q, float* means,
                                uint8_t* codes, E* out, void* ws, void* stream) {
  GRACE_REQUIRE(x && means && (codes || out) && ws && shape_ok(n, q) && SkE<E>::addressable(x) &&
                    SkE<E>::addressable(out) && al4(means) && al8(ws),
                bad);
  if (n == 0) return GRACE_OK;
  constexpr int G = SkE<E>::G;
  const hipStream_t st = as_stream(stream);
  uint8_t* w = static_cast<uint8_t*>(ws);
  float* edges = reinterpret_cast<float*>(w + kSkOffEdges);
  double* gsum = reinterpret_cast<double*>(w + kSkOffSum);
  uint32_t* gcnt = reinterpret_cast<uint32_t*>(w + kSkOffCnt);
  if (!codes) codes = w + kSkOffCodes;
  const grace_status_t s = sk_select<E>(name, x, n, q, edges, w, st);
  if (s != GRACE_OK) return s;
  const int al = al16(x) && al8(codes);
  const unsigned grid = stream_grid((n + G - 1) / G, kSkBlock, kSkGridCap);
  if (q <= 16) sk_encode_e<E, true><<<grid, kSkBlock, 0, st>>>(x, n, q, edges, codes, gsum, gcnt, al);
  else sk_encode_e<E, false><<<grid, kSkBlock, 0, st>>>(x, n, q, edges, codes, gsum, gcnt, al);
  GRACE_CHECK_LAUNCH(name);
  sk_means<<<1, kSkBlock, 0, st>>>(gsum, gcnt, q, means);
  GRACE_CHECK_LAUNCH(name);
  if (!out) return GRACE_OK;
  return sk_launch_decode<E>(name, codes, 0, means, 1, n, q, 1.0f, out, st);
}

template <typename O>
static grace_status_t sk_decode(const char* name, const char* bad, const uint8_t* codes, int64_t stride,
                                const float* means, int32_t world, int64_t n, int32_t q, float divisor, O* out,
                                void* stream) {
  GRACE_REQUIRE(codes && means && out && world >= 1 && world <= 1024 && shape_ok(n, q) && divisor != 0.0f &&
                    (world == 1 || stride >= code_bytes(n, q)) && al4(means) && SkE<O>::addressable(out),
                bad);
  if (n == 0) return GRACE_OK;
  return sk_launch_decode<O>(name, codes, stride, means, world, n, q, divisor, out, as_stream(stream));
}

}  // namespace grace

using namespace grace;

extern "C" {

size_t grace_sketch_workspace_bytes(int64_t n, int32_t q) {
  return shape_ok(n, q) ? kSkOffCodes + (size_t)code_bytes(n, q) : 0;
}

grace_status_t grace_sketch_edges(const float* x, int64_t n, int32_t q, float* edges, void* ws, void* stream) {
  return sk_edges<float>("grace_sketch_edges", "grace_sketch_edges: bad arguments", x, n, q, edges, ws, stream);
}

grace_status_t grace_sketch_edges_bf16(const uint16_t* x, int64_t n, int32_t q, float* edges, void* ws,
                                       void* stream) {
  return sk_edges<uint16_t>("grace_sketch_edges_bf16", "grace_sketch_edges_bf16: bad arguments", x, n, q, edges, ws,
                            stream);
}

grace_status_t grace_sketch_compress(const float* x, int64_t n, int32_t q, float* means, uint8_t* codes, void* ws,
                                     void* stream) {
  GRACE_REQUIRE(codes, "grace_sketch_compress: bad arguments");
  return sk_encode<float>("grace_sketch_compress", "grace_sketch_compress: bad arguments", x, n, q, means, codes,
                          nullptr, ws, stream);
}

grace_status_t grace_sketch_compress_bf16(const uint16_t* x, int64_t n, int32_t q, float* means, uint8_t* codes,
                                          void* ws, void* stream) {
  GRACE_REQUIRE(codes, "grace_sketch_compress_bf16: bad arguments");
  return sk_encode<uint16_t>("grace_sketch_compress_bf16", "grace_sketch_compress_bf16: bad arguments", x, n, q, means,
                             codes, nullptr, ws, stream);
}

grace_status_t grace_sketch_step_w1(const float* x, int64_t n, int32_t q, float* means, float* out, void* ws,
                                    void* stream) {
  GRACE_REQUIRE(out, "grace_sketch_step_w1: bad arguments");
  return sk_encode<float>("grace_sketch_step_w1", "grace_sketch_step_w1: bad arguments", x, n, q, means, nullptr, out,
                          ws, stream);
}

grace_status_t grace_sketch_step_w1_bf16(const uint16_t* x, int64_t n, int32_t q, float* means, uint16_t* out,
                                         void* ws, void* stream) {
  GRACE_REQUIRE(out, "grace_sketch_step_w1_bf16: bad arguments");
  return sk_encode<uint16_t>("grace_sketch_step_w1_bf16", "grace_sketch_step_w1_bf16: bad arguments", x, n, q, means,
                             nullptr, out, ws, stream);
}

grace_status_t grace_sketch_decode_aggregate(const uint8_t* codes, int64_t code_stride_bytes, const float* means,
                                             int32_t world, int64_t n, int32_t q, float divisor, float* out,
                                             void* stream) {
  return sk_decode<float>("grace_sketch_decode_aggregate", "grace_sketch_decode_aggregate: bad arguments", codes,
                          code_stride_bytes, means, world, n, q, divisor, out, stream);
}

grace_status_t grace_sketch_decode_aggregate_bf16(const uint8_t* codes, int64_t code_stride_bytes,
                                                  const float* means, int32_t world, int64_t n, int32_t q,
                                                  float divisor, uint16_t* out, void* stream) {
  return sk_decode<uint16_t>("grace_sketch_decode_aggregate_bf16", "grace_sketch_decode_aggregate_bf16: bad arguments",
                             codes, code_stride_bytes, means, world, n, q, divisor, out, stream);
}

}  // extern "C"
