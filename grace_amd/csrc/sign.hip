// The sign family on bfloat16 gradients, and the fused EF-signSGD step.
//
// Every kernel here is templated on the gradient's element type E: float, or uint16_t holding the
// 16 bits of a bfloat16.  A bf16 gradient is widened exactly on load (common.h bf16_to_f32) and a
// bf16 dense result is rounded once on store (f32_to_bf16, nearest even); every f32 in between --
// the EF residual, the Signum momentum, the mean -- is what the f32 kernels of elementwise.hip and
// wire.hip give for the widened gradient.  Those kernels are not touched: this file has a small
// streaming driver of its own, which keeps kU quads per lane in flight before the first use.
//
// EF-signSGD (grace_dl/dist/compressor/efsignsgd.py:12-33, memory/efsignsgd.py:9-19) as two passes:
//   A  sum |t| over the bucket, t = r + lr_mem * g formed on the fly, f64 partials per workgroup;
//   B  every workgroup sums the partials in one fixed order (workgroup 0 stores the mean), re-forms
//      t, and writes r' = t - mean * (2 c - 1) over r, optionally the u8 codes and the dense
//      world-1 result (0 + dec) / lr_agg.
// World > 1 decodes and aggregates all ranks' (mean, codes) payloads in one launch.
#include "common.h"

#include "../../include/grace_hip_sign.h"

namespace grace {

constexpr int kSBlock = 256;
constexpr int kU = 4;             // quads per lane per trip, all loaded before the first is used
constexpr int kEfParts = 2048;    // stream_grid's cap: the most f64 partials pass A can write

// ------------------------------------------------------------------------------------------------
// Element access: a quad is one 16-B (f32) or one 8-B (bf16) load or store.
template <typename E>
struct Elem;

template <>
struct Elem<float> {
  typedef float4 Raw;
  static bool aligned(const void* p) { return al16(p); }
  static bool addressable(const void*) { return true; }
  static __device__ __forceinline__ Raw ldq(const float* p, int64_t i4) {
    return reinterpret_cast<const float4*>(p)[i4];
  }
  static __device__ __forceinline__ float4 widen(Raw v) { return v; }
  static __device__ __forceinline__ float ld(const float* p, int64_t i) { return p[i]; }
  static __device__ __forceinline__ void stq(float* p, int64_t i4, float4 v) { reinterpret_cast<float4*>(p)[i4] = v; }
  static __device__ __forceinline__ void st(float* p, int64_t i, float v) { p[i] = v; }
};

template <>
struct Elem<uint16_t> {
  typedef uint2 Raw;
  static bool aligned(const void* p) { return al8(p); }
  static bool addressable(const void* p) { return al2(p); }
  static __device__ __forceinline__ Raw ldq(const uint16_t* p, int64_t i4) {
    return reinterpret_cast<const uint2*>(p)[i4];
  }
  static __device__ __forceinline__ float4 widen(Raw v) {
    return make_float4(u2f(v.x << 16), u2f(v.x & 0xFFFF0000u), u2f(v.y << 16), u2f(v.y & 0xFFFF0000u));
  }
  static __device__ __forceinline__ float ld(const uint16_t* p, int64_t i) { return bf16_to_f32(p[i]); }
  static __device__ __forceinline__ void stq(uint16_t* p, int64_t i4, float4 v) {
    reinterpret_cast<uint2*>(p)[i4] = make_uint2(pack_bf16x2(v.x, v.y), pack_bf16x2(v.z, v.w));
  }
  static __device__ __forceinline__ void st(uint16_t* p, int64_t i, float v) { p[i] = f32_to_bf16(v); }
};

__device__ __forceinline__ uint32_t ge0x4(float4 x) {
  return (uint32_t)(x.x >= 0.f) | ((uint32_t)(x.y >= 0.f) << 8) | ((uint32_t)(x.z >= 0.f) << 16) |
         ((uint32_t)(x.w >= 0.f) << 24);
}
__device__ __forceinline__ float pm1(bool p) { return p ? 1.f : -1.f; }
__device__ __forceinline__ float4 pm1x4(float4 x) {
  return make_float4(pm1(x.x >= 0.f), pm1(x.y >= 0.f), pm1(x.z >= 0.f), pm1(x.w >= 0.f));
}

// ------------------------------------------------------------------------------------------------
// Streaming driver.  Op::load(i4) issues quad i4's loads and returns them as Op::Q; Op::use(i4, q)
// computes and stores; Op::one(i) is the guarded scalar form (unaligned views, the n % 4 tail).
// A lane's kU quads of a trip are a grid stride apart, so every load instruction stays coalesced.
template <bool VEC, typename Op>
__global__ __launch_bounds__(kSBlock) void quad_kernel(Op op, int64_t n) {
  const int64_t stride = (int64_t)gridDim.x * kSBlock;
  const int64_t gid = (int64_t)blockIdx.x * kSBlock + threadIdx.x;
  if constexpr (VEC) {
    const int64_t n4 = n >> 2;
    for (int64_t b = gid; b < n4; b += stride * kU) {
      typename Op::Q q[kU];
#pragma unroll
      for (int u = 0; u < kU; ++u) {
        const int64_t i = b + u * stride;
        q[u] = op.load(i < n4 ? i : b);
      }
#pragma unroll
      for (int u = 0; u < kU; ++u) {
        const int64_t i = b + u * stride;
        if (i < n4) op.use(i, q[u]);
      }
    }
    for (int64_t i = (n4 << 2) + gid; i < n; i += stride) op.one(i);
  } else {
    for (int64_t i = gid; i < n; i += stride) op.one(i);
  }
}

static inline unsigned quad_grid(int64_t n, bool vec) {
  return vec ? stream_grid(((n >> 2) + kU - 1) / kU, kSBlock) : stream_grid(n, kSBlock);
}

template <typename Op>
static grace_status_t launch_quads(const char* name, Op op, int64_t n, bool vec, void* stream) {
  if (n <= 0) return GRACE_OK;
  if (vec) {
    quad_kernel<true, Op><<<quad_grid(n, true), kSBlock, 0, as_stream(stream)>>>(op, n);
  } else {
    quad_kernel<false, Op><<<quad_grid(n, false), kSBlock, 0, as_stream(stream)>>>(op, n);
  }
  GRACE_CHECK_LAUNCH(name);
  return GRACE_OK;
}

// ------------------------------------------------------------------------------------------------
// signSGD / Signum on E (elementwise.hip's SignEncOp, SignStepOp, SignMajOp, SignumOp)
template <typename E>
struct EncOp {
  const E* x; uint8_t* c;
  typedef typename Elem<E>::Raw Q;
  __device__ Q load(int64_t i) const { return Elem<E>::ldq(x, i); }
  __device__ void use(int64_t i, Q q) const { reinterpret_cast<uint32_t*>(c)[i] = ge0x4(Elem<E>::widen(q)); }
  __device__ void one(int64_t i) const { c[i] = (uint8_t)(Elem<E>::ld(x, i) >= 0.f); }
};

template <typename E>
struct StepOp {
  const E* x; uint8_t* c; E* o;
  typedef typename Elem<E>::Raw Q;
  __device__ Q load(int64_t i) const { return Elem<E>::ldq(x, i); }
  __device__ void use(int64_t i, Q q) const {
    const float4 v = Elem<E>::widen(q);
    if (c) reinterpret_cast<uint32_t*>(c)[i] = ge0x4(v);
    Elem<E>::stq(o, i, pm1x4(v));
  }
  __device__ void one(int64_t i) const {
    const bool p = Elem<E>::ld(x, i) >= 0.f;
    if (c) c[i] = (uint8_t)p;
    Elem<E>::st(o, i, pm1(p));
  }
};

// World-1 step without codes, every load before any store and no loop (elementwise.hip's
// sign_step_w1_kernel: the launch-bound sizes); the n % 4 tail goes to the first workgroup.
template <int U, typename E>
__global__ __launch_bounds__(kSBlock) void step_w1_kernel(const E* __restrict__ x, E* __restrict__ o, int64_t n) {
  const int64_t n4 = n >> 2;
  const int64_t base = (int64_t)blockIdx.x * kSBlock * U + threadIdx.x;
  typename Elem<E>::Raw v[U];
#pragma unroll
  for (int u = 0; u < U; ++u) {
    const int64_t i = base + (int64_t)u * kSBlock;
    v[u] = Elem<E>::ldq(x, i < n4 ? i : 0);
  }
#pragma unroll
  for (int u = 0; u < U; ++u) {
    const int64_t i = base + (int64_t)u * kSBlock;
    if (i < n4) Elem<E>::stq(o, i, pm1x4(Elem<E>::widen(v[u])));
  }
  if (blockIdx.x == 0 && threadIdx.x < (n & 3)) {
    const int64_t i = (n4 << 2) + threadIdx.x;
    Elem<E>::st(o, i, pm1(Elem<E>::ld(x, i) >= 0.f));
  }
}

// majority over W rank-major u8 rows: the f32 sum of +-1 in rank order (exact), >= 0 -> +1
template <typename E>
struct MajOp {
  const uint8_t* c; int world; int64_t n; E* o;
  struct Q {};
  __device__ Q load(int64_t) const { return Q{}; }
  __device__ void use(int64_t i, Q) const {
    float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
    for (int w = 0; w < world; ++w) {
      const uint32_t v = reinterpret_cast<const uint32_t*>(c + (int64_t)w * n)[i];
      s0 += (float)(v & 0xFF) * 2.f - 1.f; s1 += (float)((v >> 8) & 0xFF) * 2.f - 1.f;
      s2 += (float)((v >> 16) & 0xFF) * 2.f - 1.f; s3 += (float)(v >> 24) * 2.f - 1.f;
    }
    Elem<E>::stq(o, i, pm1x4(make_float4(s0, s1, s2, s3)));
  }
  __device__ void one(int64_t i) const {
    float s = 0.f;
    for (int w = 0; w < world; ++w) s += (float)c[(int64_t)w * n + i] * 2.f - 1.f;
    Elem<E>::st(o, i, pm1(s >= 0.f));
  }
};

// Signum: m = a g + b m_prev in f32 (m = g on the first step), codes = (m >= 0)
template <typename E>
struct SignumOp {
  const E* g; float* m; int has_prev; float a, b; uint8_t* c;
  struct Q { typename Elem<E>::Raw g; float4 m; };
  __device__ float upd(float gv, float mv) const { return has_prev ? a * gv + b * mv : gv; }
  __device__ Q load(int64_t i) const {
    Q q;
    q.g = Elem<E>::ldq(g, i);
    q.m = has_prev ? reinterpret_cast<const float4*>(m)[i] : make_float4(0.f, 0.f, 0.f, 0.f);
    return q;
  }
  __device__ void use(int64_t i, const Q& q) const {
    const float4 gv = Elem<E>::widen(q.g);
    const float4 o = make_float4(upd(gv.x, q.m.x), upd(gv.y, q.m.y), upd(gv.z, q.m.z), upd(gv.w, q.m.w));
    reinterpret_cast<float4*>(m)[i] = o;
    reinterpret_cast<uint32_t*>(c)[i] = ge0x4(o);
  }
  __device__ void one(int64_t i) const {
    const float o = upd(Elem<E>::ld(g, i), has_prev ? m[i] : 0.f);
    m[i] = o;
    c[i] = (uint8_t)(o >= 0.f);
  }
};

// ------------------------------------------------------------------------------------------------
// 1-bit wire (wire.hip's sign_encode_bits_kernel and majority_bits_kernel) on E.  Lane l of a wave
// owns elements base + 4 l .. + 3; four ballots collect a 256-element slice's codes and lanes 0..7
// store its 8 words.
__device__ __forceinline__ uint32_t spread_nib(uint32_t b) {   // bit i of b (i < 8) -> bit 4 i
  b = (b | (b << 12)) & 0x000F000Fu;
  b = (b | (b << 6)) & 0x03030303u;
  b = (b | (b << 3)) & 0x11111111u;
  return b;
}

template <typename E>
__global__ __launch_bounds__(kSBlock) void encode_bits_kernel(const E* __restrict__ x, int64_t n,
                                                              uint32_t* __restrict__ words, bool vec) {
  const int lane = threadIdx.x & 63;
  const int64_t nwaves = (int64_t)gridDim.x * (kSBlock / 64);
  const int64_t wave = (int64_t)blockIdx.x * (kSBlock / 64) + (threadIdx.x >> 6);
  const int64_t nw = (n + 31) >> 5;
  for (int64_t base = wave * 256 * kU; base < n; base += nwaves * 256 * kU) {
    float4 v[kU];
#pragma unroll
    for (int u = 0; u < kU; ++u) {
      const int64_t e = base + 256 * u + 4 * lane;
      if (vec && e + 3 < n) {
        v[u] = Elem<E>::widen(Elem<E>::ldq(x, e >> 2));
      } else {   // past n: code 0
        v[u].x = e < n ? Elem<E>::ld(x, e) : -1.f;
        v[u].y = e + 1 < n ? Elem<E>::ld(x, e + 1) : -1.f;
        v[u].z = e + 2 < n ? Elem<E>::ld(x, e + 2) : -1.f;
        v[u].w = e + 3 < n ? Elem<E>::ld(x, e + 3) : -1.f;
      }
    }
#pragma unroll
    for (int u = 0; u < kU; ++u) {
      const uint64_t b0 = __ballot(v[u].x >= 0.f), b1 = __ballot(v[u].y >= 0.f);
      const uint64_t b2 = __ballot(v[u].z >= 0.f), b3 = __ballot(v[u].w >= 0.f);
      if (lane < 8) {
        const int sh = 8 * lane;
        const uint32_t wd = spread_nib((uint32_t)(b0 >> sh) & 0xFFu) | (spread_nib((uint32_t)(b1 >> sh) & 0xFFu) << 1) |
                            (spread_nib((uint32_t)(b2 >> sh) & 0xFFu) << 2) |
                            (spread_nib((uint32_t)(b3 >> sh) & 0xFFu) << 3);
        const int64_t wi = ((base + 256 * u) >> 5) + lane;
        if (wi < nw) words[wi] = wd;
      }
    }
  }
}

template <typename E>
__global__ __launch_bounds__(kSBlock) void majority_bits_kernel_e(const uint32_t* __restrict__ words, int64_t stride,
                                                                  int world, int64_t n, E* __restrict__ out, bool vec) {
  const int lane = threadIdx.x & 63;
  const int64_t nwaves = (int64_t)gridDim.x * (kSBlock / 64);
  const int64_t wave = (int64_t)blockIdx.x * (kSBlock / 64) + (threadIdx.x >> 6);
  for (int64_t base = wave * 256 * kU; base < n; base += nwaves * 256 * kU) {
    uint32_t ones[kU][4] = {};
    for (int r = 0; r < world; ++r) {
      uint32_t wv[kU];
#pragma unroll
      for (int u = 0; u < kU; ++u) {   // every word of the round in flight before any is used
        const int64_t e = base + 256 * u + 4 * lane;
        wv[u] = e < n ? words[r * stride + (e >> 5)] : 0u;
      }
#pragma unroll
      for (int u = 0; u < kU; ++u) {
        const uint32_t nib = wv[u] >> (4 * (lane & 7));
#pragma unroll
        for (int j = 0; j < 4; ++j) ones[u][j] += (nib >> j) & 1u;
      }
    }
#pragma unroll
    for (int u = 0; u < kU; ++u) {
      const int64_t e = base + 256 * u + 4 * lane;
      float v[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) v[j] = pm1(2 * (int)ones[u][j] - world >= 0);
      if (vec && e + 3 < n) {
        Elem<E>::stq(out, e >> 2, make_float4(v[0], v[1], v[2], v[3]));
      } else {
#pragma unroll
        for (int j = 0; j < 4; ++j)
          if (e + j < n) Elem<E>::st(out, e + j, v[j]);
      }
    }
  }
}

// ------------------------------------------------------------------------------------------------
// EF-signSGD.  t = r + lr * g: the product rounds, then the sum (no contraction), which is
// grace_axpby(r, g, 1.0, lr) since 1.0 * r is exact; a name's first step has t = g.
template <typename E>
struct EfIn {
  const E* g; const float* r; int has; float lr;
  struct Q { typename Elem<E>::Raw g; float4 r; };
  __device__ __forceinline__ Q load(int64_t i) const {
    Q q;
    q.g = Elem<E>::ldq(g, i);
    q.r = has ? reinterpret_cast<const float4*>(r)[i] : make_float4(0.f, 0.f, 0.f, 0.f);
    return q;
  }
  __device__ __forceinline__ float t1(float gv, float rv) const { return has ? rv + lr * gv : gv; }
  __device__ __forceinline__ float4 t(const Q& q) const {
    const float4 gv = Elem<E>::widen(q.g);
    return make_float4(t1(gv.x, q.r.x), t1(gv.y, q.r.y), t1(gv.z, q.r.z), t1(gv.w, q.r.w));
  }
  __device__ __forceinline__ float tone(int64_t i) const { return t1(Elem<E>::ld(g, i), has ? r[i] : 0.f); }
};

// Sum over the workgroup, the same bits in every thread: xor butterflies inside each wave (both
// partners add the same two operands), then the four wave totals in wave order.
__device__ __forceinline__ double block_sum(double v) {
  __shared__ double sh[kSBlock / kWave];
  v = wave_sum(v);
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
  __syncthreads();
  double t = 0.0;
#pragma unroll
  for (int w = 0; w < kSBlock / kWave; ++w) t += sh[w];
  return t;
}

// Pass A: part[workgroup] = sum of |t| over the workgroup's elements, in f64.  The partition and
// the order of every addition depend only on (n, the path), so two calls give the same bits.
template <bool VEC, typename E>
__global__ __launch_bounds__(kSBlock) void ef_sum_kernel(EfIn<E> in, int64_t n, double* __restrict__ part) {
  const int64_t stride = (int64_t)gridDim.x * kSBlock;
  const int64_t gid = (int64_t)blockIdx.x * kSBlock + threadIdx.x;
  double s = 0.0;
  if constexpr (VEC) {
    const int64_t n4 = n >> 2;
    for (int64_t b = gid; b < n4; b += stride * kU) {
      typename EfIn<E>::Q q[kU];
#pragma unroll
      for (int u = 0; u < kU; ++u) {
        const int64_t i = b + u * stride;
        q[u] = in.load(i < n4 ? i : b);
      }
#pragma unroll
      for (int u = 0; u < kU; ++u) {
        if (b + u * stride < n4) {
          const float4 t = in.t(q[u]);
          s += (double)fabsf(t.x); s += (double)fabsf(t.y); s += (double)fabsf(t.z); s += (double)fabsf(t.w);
        }
      }
    }
    for (int64_t i = (n4 << 2) + gid; i < n; i += stride) s += (double)fabsf(in.tone(i));
  } else {
    for (int64_t i = gid; i < n; i += stride) s += (double)fabsf(in.tone(i));
  }
  s = block_sum(s);
  if (threadIdx.x == 0) part[blockIdx.x] = s;
}

// What pass B writes per element, given the mean: dec = mean * (2 c - 1) takes two values, and so
// does the dense result (0 + dec) / lr_agg, so both are formed once per lane (one IEEE division
// each) and selected per element.
struct EfVals {
  float dec0, dec1, res0, res1;   // by code (selected, never indexed: no scratch)
  __device__ __forceinline__ EfVals(float mean, float lr_agg) {
    dec0 = mean * (0.0f * 2.0f - 1.0f);
    dec1 = mean * (1.0f * 2.0f - 1.0f);
    res0 = (0.f + dec0) / lr_agg;
    res1 = (0.f + dec1) / lr_agg;
  }
  __device__ __forceinline__ float dec(bool c) const { return c ? dec1 : dec0; }
  __device__ __forceinline__ float res(bool c) const { return c ? res1 : res0; }
};

template <bool VEC, typename E>
__global__ __launch_bounds__(kSBlock) void ef_apply_kernel(EfIn<E> in, int64_t n, const double* __restrict__ part,
                                                           int nparts, float* __restrict__ mean_out,
                                                           float* r_out, uint8_t* __restrict__ codes,
                                                           E* __restrict__ out, float lr_agg) {
  const int64_t stride = (int64_t)gridDim.x * kSBlock;
  const int64_t gid = (int64_t)blockIdx.x * kSBlock + threadIdx.x;
  const int64_t n4 = VEC ? n >> 2 : 0;
  // the first trip's loads are issued before the partials are summed
  typename EfIn<E>::Q q[kU];
  if constexpr (VEC) {
    if (gid < n4) {
#pragma unroll
      for (int u = 0; u < kU; ++u) {
        const int64_t i = gid + u * stride;
        q[u] = in.load(i < n4 ? i : gid);
      }
    }
  }
  double s = 0.0;
  for (int b = threadIdx.x; b < nparts; b += kSBlock) s += part[b];
  const float mean = (float)block_sum(s) / (float)n;
  if (gid == 0) mean_out[0] = mean;
  const EfVals v(mean, lr_agg);

  if constexpr (VEC) {
    for (int64_t b = gid; b < n4;) {
#pragma unroll
      for (int u = 0; u < kU; ++u) {
        const int64_t i = b + u * stride;
        if (i < n4) {
          const float4 t = in.t(q[u]);
          const bool c0 = t.x >= 0.f, c1 = t.y >= 0.f, c2 = t.z >= 0.f, c3 = t.w >= 0.f;
          reinterpret_cast<float4*>(r_out)[i] =
              make_float4(t.x - v.dec(c0), t.y - v.dec(c1), t.z - v.dec(c2), t.w - v.dec(c3));
          if (codes)
            reinterpret_cast<uint32_t*>(codes)[i] =
                (uint32_t)c0 | ((uint32_t)c1 << 8) | ((uint32_t)c2 << 16) | ((uint32_t)c3 << 24);
          if (out) Elem<E>::stq(out, i, make_float4(v.res(c0), v.res(c1), v.res(c2), v.res(c3)));
        }
      }
      b += stride * kU;
      if (b < n4) {
#pragma unroll
        for (int u = 0; u < kU; ++u) {
          const int64_t i = b + u * stride;
          q[u] = in.load(i < n4 ? i : b);
        }
      }
    }
  }
  for (int64_t i = (n4 << 2) + gid; i < n; i += stride) {
    const float t = in.tone(i);
    const bool c = t >= 0.f;
    r_out[i] = t - v.dec(c);
    if (codes) codes[i] = (uint8_t)c;
    if (out) Elem<E>::st(out, i, v.res(c));
  }
}

// World > 1: out = (((0 + m_0 d_0) + m_1 d_1) + ...) / lr_agg over the gathered payloads, rank w's
// codes at + w * n.  Four ranks' code words are loaded before the first is used.
template <typename E>
struct EfDecOp {
  const float* means; const uint8_t* c; int world; int64_t n; float lr_agg; E* o;
  struct Q {};
  __device__ Q load(int64_t) const { return Q{}; }
  static __device__ __forceinline__ float dec(float m, uint32_t b) { return m * ((float)b * 2.0f - 1.0f); }
  __device__ __forceinline__ void add(float4& s, float m, uint32_t v) const {
    s.x += dec(m, v & 0xFF); s.y += dec(m, (v >> 8) & 0xFF); s.z += dec(m, (v >> 16) & 0xFF); s.w += dec(m, v >> 24);
  }
  __device__ void use(int64_t i, Q) const {
    float4 s = make_float4(0.f, 0.f, 0.f, 0.f);
    const uint32_t* row = reinterpret_cast<const uint32_t*>(c) + i;   // n % 4 == 0: every row stays aligned
    const int64_t rs = n >> 2;
    int w = 0;
    for (; w + 4 <= world; w += 4) {
      const uint32_t v0 = row[w * rs], v1 = row[(w + 1) * rs], v2 = row[(w + 2) * rs], v3 = row[(w + 3) * rs];
      add(s, means[w], v0); add(s, means[w + 1], v1); add(s, means[w + 2], v2); add(s, means[w + 3], v3);
    }
    for (; w < world; ++w) add(s, means[w], row[w * rs]);
    Elem<E>::stq(o, i, make_float4(s.x / lr_agg, s.y / lr_agg, s.z / lr_agg, s.w / lr_agg));
  }
  __device__ void one(int64_t i) const {
    float s = 0.f;
    for (int w = 0; w < world; ++w) s += dec(means[w], c[(int64_t)w * n + i]);
    Elem<E>::st(o, i, s / lr_agg);
  }
};

// ------------------------------------------------------------------------------------------------
// host side
template <typename E>
static grace_status_t efsign_step(const char* name, const char* bad, const E* g, float* residual, int32_t has,
                                  float lr_mem, int64_t n, float* mean_out, uint8_t* codes, E* out, float lr_agg,
                                  void* ws, size_t ws_bytes, void* stream) {
  GRACE_REQUIRE(g && residual && mean_out && ws && n >= 0 && ws_bytes >= grace_efsign_workspace_bytes(n) &&
                    Elem<E>::addressable(g) && Elem<E>::addressable(out),
                bad);
  if (n == 0) return GRACE_OK;
  const bool vec = Elem<E>::aligned(g) && al16(residual) && (!codes || al4(codes)) && (!out || Elem<E>::aligned(out));
  const EfIn<E> in{g, residual, has ? 1 : 0, lr_mem};
  double* part = reinterpret_cast<double*>(ws);
  const unsigned grid = quad_grid(n, vec);   // <= kEfParts
  if (vec) {
    ef_sum_kernel<true, E><<<grid, kSBlock, 0, as_stream(stream)>>>(in, n, part);
    GRACE_CHECK_LAUNCH(name);
    ef_apply_kernel<true, E><<<grid, kSBlock, 0, as_stream(stream)>>>(in, n, part, (int)grid, mean_out, residual, codes,
                                                                      out, lr_agg);
  } else {
    ef_sum_kernel<false, E><<<grid, kSBlock, 0, as_stream(stream)>>>(in, n, part);
    GRACE_CHECK_LAUNCH(name);
    ef_apply_kernel<false, E><<<grid, kSBlock, 0, as_stream(stream)>>>(in, n, part, (int)grid, mean_out, residual,
                                                                       codes, out, lr_agg);
  }
  GRACE_CHECK_LAUNCH(name);
  return GRACE_OK;
}

template <typename E>
static grace_status_t efsign_decode(const char* name, const char* bad, const float* means, const uint8_t* codes_wn,
                                    int32_t world, float lr_agg, E* out, int64_t n, void* stream) {
  GRACE_REQUIRE(means && codes_wn && out && world >= 1 && n >= 0 && Elem<E>::addressable(out), bad);
  const bool vec = al4(codes_wn) && (world == 1 || n % 4 == 0) && Elem<E>::aligned(out);
  return launch_quads(name, EfDecOp<E>{means, codes_wn, world, n, lr_agg, out}, n, vec, stream);
}

}  // namespace grace

using namespace grace;

extern "C" {

size_t grace_efsign_workspace_bytes(int64_t n) {
  (void)n;
  return sizeof(double) * kEfParts;
}

grace_status_t grace_efsign_step(const float* g, float* residual, int32_t has_residual, float lr_mem, int64_t n,
                                 float* mean_out, uint8_t* codes, float* out, float lr_agg, void* ws, size_t ws_bytes,
                                 void* stream) {
  return efsign_step<float>("grace_efsign_step", "grace_efsign_step: bad arguments", g, residual, has_residual, lr_mem,
                            n, mean_out, codes, out, lr_agg, ws, ws_bytes, stream);
}

grace_status_t grace_efsign_step_bf16(const uint16_t* g, float* residual, int32_t has_residual, float lr_mem, int64_t n,
                                      float* mean_out, uint8_t* codes, uint16_t* out, float lr_agg, void* ws,
                                      size_t ws_bytes, void* stream) {
  return efsign_step<uint16_t>("grace_efsign_step_bf16", "grace_efsign_step_bf16: bad arguments", g, residual,
                               has_residual, lr_mem, n, mean_out, codes, out, lr_agg, ws, ws_bytes, stream);
}

grace_status_t grace_efsign_decode_aggregate(const float* means, const uint8_t* codes_wn, int32_t world, float lr_agg,
                                             float* out, int64_t n, void* stream) {
  return efsign_decode<float>("grace_efsign_decode_aggregate", "grace_efsign_decode_aggregate: bad arguments", means,
                              codes_wn, world, lr_agg, out, n, stream);
}

grace_status_t grace_efsign_decode_aggregate_bf16(const float* means, const uint8_t* codes_wn, int32_t world,
                                                  float lr_agg, uint16_t* out, int64_t n, void* stream) {
  return efsign_decode<uint16_t>("grace_efsign_decode_aggregate_bf16",
                                 "grace_efsign_decode_aggregate_bf16: bad arguments", means, codes_wn, world, lr_agg,
                                 out, n, stream);
}

grace_status_t grace_sign_encode_bf16(const uint16_t* x, uint8_t* codes, int64_t n, void* stream) {
  GRACE_REQUIRE(n >= 0 && x && codes && al2(x), "grace_sign_encode_bf16: bad arguments");
  return launch_quads("grace_sign_encode_bf16", EncOp<uint16_t>{x, codes}, n, al8(x) && al4(codes), stream);
}

grace_status_t grace_sign_encode_bits_bf16(const uint16_t* x, int64_t n, uint32_t* words, void* stream) {
  GRACE_REQUIRE(x && words && n >= 0 && al2(x), "grace_sign_encode_bits_bf16: bad arguments");
  if (n == 0) return GRACE_OK;
  encode_bits_kernel<uint16_t><<<stream_grid((n + 1023) / 1024, kU, 4096), kSBlock, 0, as_stream(stream)>>>(
      x, n, words, al8(x));
  GRACE_CHECK_LAUNCH("grace_sign_encode_bits_bf16");
  return GRACE_OK;
}

grace_status_t grace_sign_step_w1_bf16(const uint16_t* x, uint8_t* codes, uint16_t* out, int64_t n, void* stream) {
  GRACE_REQUIRE(n >= 0 && x && out && al2(x) && al2(out), "grace_sign_step_w1_bf16: bad arguments");
  if (!codes && n >= 4 && al8(x) && al8(out)) {
    constexpr int U = 1;   // as grace_sign_step_w1
    const int64_t grid = ((n >> 2) + kSBlock * U - 1) / (kSBlock * U);
    step_w1_kernel<U, uint16_t><<<(unsigned)grid, kSBlock, 0, as_stream(stream)>>>(x, out, n);
    GRACE_CHECK_LAUNCH("grace_sign_step_w1_bf16");
    return GRACE_OK;
  }
  return launch_quads("grace_sign_step_w1_bf16", StepOp<uint16_t>{x, codes, out}, n,
                      al8(x) && (!codes || al4(codes)) && al8(out), stream);
}

grace_status_t grace_sign_majority_bf16(const uint8_t* codes_wn, int32_t world, uint16_t* out, int64_t n,
                                        void* stream) {
  GRACE_REQUIRE(n >= 0 && world >= 1 && codes_wn && out && al2(out), "grace_sign_majority_bf16: bad arguments");
  return launch_quads("grace_sign_majority_bf16", MajOp<uint16_t>{codes_wn, world, n, out}, n,
                      al4(codes_wn) && (n % 4 == 0) && al8(out), stream);
}

grace_status_t grace_sign_majority_bits_bf16(const uint32_t* words, int64_t stride_words, int32_t world, int64_t n,
                                             uint16_t* out, void* stream) {
  GRACE_REQUIRE(words && out && world >= 1 && world <= 63 && n >= 0 && al2(out),
                "grace_sign_majority_bits_bf16: bad arguments");
  if (n == 0) return GRACE_OK;
  majority_bits_kernel_e<uint16_t><<<stream_grid((n + 1023) / 1024, kU, 4096), kSBlock, 0, as_stream(stream)>>>(
      words, stride_words, world, n, out, al8(out));
  GRACE_CHECK_LAUNCH("grace_sign_majority_bits_bf16");
  return GRACE_OK;
}

grace_status_t grace_signum_encode_bf16(const uint16_t* g, float* momentum, int32_t has_prev, float coef_g,
                                        float coef_m, uint8_t* codes, int64_t n, void* stream) {
  GRACE_REQUIRE(n >= 0 && g && momentum && codes && al2(g), "grace_signum_encode_bf16: bad arguments");
  return launch_quads("grace_signum_encode_bf16", SignumOp<uint16_t>{g, momentum, has_prev, coef_g, coef_m, codes}, n,
                      al8(g) && al16(momentum) && al4(codes), stream);
}

}  // extern "C"
