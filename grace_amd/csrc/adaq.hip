// Adaptive quantisation (AdaQ; include/grace_hip_adaq.h): an exact top-k of each sign
// class, sent as 2-byte {sign, offset} entries behind a chunk directory and two means.
//
// Everything is integer work on the bit patterns: mag = u & 0x7FFFFFFF orders the magnitudes, u >> 31
// is the class (mag == 0 belongs to none).  The tensor is cut into chunks of 8192 elements.
//
//   select   T+ and T- together, exactly, by radix passes over the 31 magnitude bits, digits of
//            11 / 10 / 10 bits from the top.  A pass is a grid-stride sweep: every workgroup keeps one
//            LDS histogram per sign (16 KB, then 8 KB) and flushes its non-zero bins with integer
//            atomics; between passes one workgroup walks both histograms from the top
//            (find_bin_desc).  The class sizes fall out of pass 0 and k+ and k- are computed there,
//            on the device.  f32 is read three times; a bf16 magnitude has 15 bits, so the second
//            pass already ends at bit 16 and bf16 is read twice.  Whatever the data.
//   count    one workgroup a chunk: per sign the number above the cut, the number at the cut and the
//            f64 sum of the elements above it, reduced over the workgroup in a fixed tree; one
//            32-byte record a chunk, plain stores.
//   scan     one workgroup over the records in chunk order: each chunk's tie base per sign, the ties
//            it takes, the directory, the two means, the header, the zero tail and the padding.
//   place    one workgroup a chunk re-reads it with coalesced 16-byte loads and turns the flags
//            {above, tie, sign} into three bit masks in LDS, 32 elements a word and one word a thread
//            (a lane's 4 or 8 flags are OR-ed across the 8 or 4 lanes of a word with shuffles).  A
//            scan of the words' tie counts picks the ties to take; a scan of the words' selected
//            counts places every entry in element order.  The entries are staged in LDS at the
//            destination's phase mod 16 B and leave in 16-byte stores; the at most 7 entries at
//            either end that share a 16-byte line with a neighbour chunk go as 2-byte stores.  No
//            workgroup waits for another and no two write one address.
//   step     world 1: select, count and scan as above (no payload), then the place kernel's mask and
//            tie phases, after which every lane writes 16 B of the result from the masks and the means.
//   decode   one workgroup a chunk of the output holds 8192 f32 accumulators in LDS (32 KB) and
//            applies rank after rank to them, a barrier between two ranks, so the sum is in rank
//            order; inside one rank the entries of a chunk have distinct offsets and need no atomics.
//            The tile then leaves in 16-byte stores as f32 or bf16.
//
// Operands off their 16-byte grid and the ragged chunk go through guarded per-element accesses in the
// same kernels.
#include "select.h"

#include "../../include/grace_hip_adaq.h"

namespace grace {

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

constexpr int kAqChunk = 8192;
constexpr int kAqBlock = 256;                     // count, place and decode: one workgroup a chunk
constexpr int kAqWaves = kAqBlock / kWave;
constexpr int kAqWords = kAqChunk / 32;           // flag words a chunk
constexpr int kAqSelBlock = 1024;                 // histogram passes, resolve and scan: 16 waves
constexpr int kAqSelWaves = kAqSelBlock / kWave;
constexpr int kAqSelGridCap = 512;                // one sweep = 2^21 f32 / 2^22 bf16 elements
constexpr int kAqBins0 = 2048, kAqBins = 1024;    // digits of 11, 10 and 10 bits
static_assert(kAqWords == kAqBlock, "one flag word a thread");

// workspace layout, in bytes: two histograms a level, the state, then a record and a tie base a chunk
constexpr size_t kAqOffHist0 = 0;                                             // u32[2][2048]
constexpr size_t kAqOffHist1 = kAqOffHist0 + sizeof(uint32_t) * 2 * kAqBins0; // u32[2][1024]
constexpr size_t kAqOffHist2 = kAqOffHist1 + sizeof(uint32_t) * 2 * kAqBins;  // u32[2][1024]
constexpr size_t kAqOffState = kAqOffHist2 + sizeof(uint32_t) * 2 * kAqBins;
constexpr size_t kAqOffRecords = kAqOffState + 256;                           // everything before is zeroed per call
constexpr size_t kAqRecordBytes = 32, kAqTieBytes = 8;
// state words, each a pair {positive, negative}
constexpr int kAqPref = 0;    // the digits found so far (0xFFFFFFFF: the class is empty)
constexpr int kAqRem = 2;     // the rank still wanted inside that prefix
constexpr int kAqK = 4;       // k_s
constexpr int kAqCut = 6;     // T_s (0xFFFFFFFF: the class is empty; no magnitude reaches it)
constexpr int kAqTake = 8;    // ties taken: k_s - #{mag > T_s}
constexpr int kAqMean = 10;   // the means' bits
constexpr uint32_t kAqNone = 0xFFFFFFFFu;

// the gradient's elements as f32 bit patterns; the dense result from f32
template <typename E>
struct AqE;
template <>
struct AqE<float> {
  static constexpr int G = 4;                     // elements in 16 B
  static bool addressable(const void* p) { return al4(p); }
  static __device__ __forceinline__ uint32_t ld(const float* p, int64_t i) { return f2u(p[i]); }
  static __device__ __forceinline__ void st(float* p, int64_t i, float v) { p[i] = v; }
  static __device__ __forceinline__ void unpack(u32x4 v, uint32_t (&u)[4]) {
#pragma unroll
    for (int j = 0; j < 4; ++j) u[j] = v[j];
  }
  static __device__ __forceinline__ u32x4 pack(const float (&d)[4]) {
    u32x4 v;
#pragma unroll
    for (int j = 0; j < 4; ++j) v[j] = f2u(d[j]);
    return v;
  }
};
template <>
struct AqE<uint16_t> {
  static constexpr int G = 8;
  static bool addressable(const void* p) { return al2(p); }
  static __device__ __forceinline__ uint32_t ld(const uint16_t* p, int64_t i) { return (uint32_t)p[i] << 16; }
  static __device__ __forceinline__ void st(uint16_t* p, int64_t i, float v) { p[i] = f32_to_bf16(v); }
  static __device__ __forceinline__ void unpack(u32x4 v, uint32_t (&u)[8]) {
#pragma unroll
    for (int j = 0; j < 4; ++j) { u[2 * j] = v[j] << 16; u[2 * j + 1] = v[j] & 0xFFFF0000u; }
  }
  static __device__ __forceinline__ u32x4 pack(const float (&d)[8]) {
    u32x4 v;
#pragma unroll
    for (int j = 0; j < 4; ++j) v[j] = pack_bf16x2(d[2 * j], d[2 * j + 1]);
    return v;
  }
};

// u[j] = the bits of x[e + j]; 0 (no class) where e + j >= n
template <typename E>
__device__ __forceinline__ void aq_load(const E* x, int64_t e, int64_t n, bool fast, uint32_t (&u)[AqE<E>::G]) {
  if (fast) {
    AqE<E>::unpack(*reinterpret_cast<const u32x4*>(x + e), u);
  } else {
#pragma unroll
    for (int j = 0; j < AqE<E>::G; ++j) u[j] = e + j < n ? AqE<E>::ld(x, e + j) : 0u;
  }
}

template <typename O>
__device__ __forceinline__ void aq_store(O* o, int64_t e, int64_t n, bool fast, const float (&d)[AqE<O>::G]) {
  if (fast) {
    __builtin_nontemporal_store(AqE<O>::pack(d), reinterpret_cast<u32x4*>(o + e));
  } else {
#pragma unroll
    for (int j = 0; j < AqE<O>::G; ++j)
      if (e + j < n) AqE<O>::st(o, e + j, d[j]);
  }
}

__device__ __forceinline__ double aq_f64(uint32_t lo, uint32_t hi) {
  return __longlong_as_double((long long)(((uint64_t)hi << 32) | lo));
}

// the lowest r set bits of w (all of them when r >= popc(w))
__device__ __forceinline__ uint32_t aq_first_bits(uint32_t w, uint32_t r) {
  if (r >= (uint32_t)__popc(w)) return w;
  uint32_t rest = w;
  for (uint32_t i = 0; i < r; ++i) rest &= rest - 1u;
  return w ^ rest;
}

static inline int64_t aq_chunks(int64_t n) { return (n + kAqChunk - 1) / kAqChunk; }
static inline int64_t aq_dir_words(int64_t n) { return (aq_chunks(n) + 3) / 4 * 4; }

// ------------------------------------------------------------------------------------------------
// two-rank select
__global__ __launch_bounds__(kAqSelBlock) void aq_zero(uint32_t* __restrict__ p, int words) {
  for (int i = blockIdx.x * kAqSelBlock + threadIdx.x; i < words; i += gridDim.x * kAqSelBlock) p[i] = 0u;
}

// One histogram pass: a class member whose bits above the digit equal its class's prefix counts in
// that class's histogram of the digit, the `bits` bits from bit `shift` up.
template <typename E>
__global__ __launch_bounds__(kAqSelBlock) void aq_hist_e(const E* __restrict__ x, int64_t n, int shift, int bits,
                                                         const uint32_t* __restrict__ state,
                                                         uint32_t* __restrict__ hist, int aligned) {
  constexpr int G = AqE<E>::G;
  __shared__ uint32_t sh_h[2 * kAqBins0];
  const uint32_t nbins = 1u << bits, pp = state[kAqPref], pn = state[kAqPref + 1];
  for (uint32_t b = threadIdx.x; b < 2u * nbins; b += kAqSelBlock) sh_h[b] = 0u;
  __syncthreads();

  const int64_t ng = (n + G - 1) / G;
#pragma unroll 2
  for (int64_t g = (int64_t)blockIdx.x * kAqSelBlock + threadIdx.x; g < ng; g += (int64_t)gridDim.x * kAqSelBlock) {
    const int64_t e = g * G;
    uint32_t u[G];
    aq_load<E>(x, e, n, aligned && e + G <= n, u);
#pragma unroll
    for (int j = 0; j < G; ++j) {
      const uint32_t m = u[j] & 0x7FFFFFFFu, s = u[j] >> 31;
      if (m != 0u && (m >> (shift + bits)) == (s ? pn : pp))
        atomicAdd(&sh_h[s * nbins + ((m >> shift) & (nbins - 1u))], 1u);
    }
  }
  __syncthreads();
  for (uint32_t b = threadIdx.x; b < 2u * nbins; b += kAqSelBlock) {
    const uint32_t c = sh_h[b];
    if (c) atomicAdd(hist + b, c);
  }
}

// Between passes, one workgroup: per sign the bin its remaining rank falls in.  first: the class
// sizes are the histograms' totals and k_s = ceil(m_s * ratio).  last_shift >= 0: the prefix is the
// cut but for that many zero bits below it (bf16 after its second pass: 10).
template <int BINS>
__global__ __launch_bounds__(kAqSelBlock) void aq_resolve(const uint32_t* __restrict__ hist, uint32_t* __restrict__ state,
                                                          double ratio, int bits, int first, int last_shift) {
  constexpr int PER = BINS / kAqSelBlock;
  __shared__ uint32_t s_w[kAqSelWaves + 1], s_res[2];
  for (int s = 0; s < 2; ++s) {
    const uint32_t* h = hist + s * BINS;
    uint32_t k = state[kAqK + s], rank = state[kAqRem + s], pref = state[kAqPref + s];
    if (first) {
      uint32_t mine = 0, m;
#pragma unroll
      for (int j = 0; j < PER; ++j) mine += h[threadIdx.x * PER + j];
      block_excl_scan<kAqSelBlock>(mine, s_w, &m);
      k = m ? (uint32_t)ceil((double)m * ratio) : 0u;
      k = min(max(k, m ? 1u : 0u), m);
      rank = k;
    }
    uint32_t above;
    const int d = find_bin_desc<kAqSelBlock, BINS>(h, max(rank, 1u), s_w, s_res, &above);
    if (threadIdx.x == 0) {
      if (k == 0u) {
        pref = kAqNone;
        rank = 0u;
      } else {
        pref = (pref << bits) | (uint32_t)d;
        rank -= above;
      }
      state[kAqK + s] = k;
      state[kAqPref + s] = pref;
      state[kAqRem + s] = rank;
      if (last_shift >= 0) {
        state[kAqCut + s] = k ? pref << last_shift : kAqNone;
        state[kAqTake + s] = rank;
      }
    }
  }
}

// ------------------------------------------------------------------------------------------------
// count pass: record = {above+, above-, ties+, ties-, f64 sum+, f64 sum-} of the chunk
template <typename E>
__global__ __launch_bounds__(kAqBlock) void aq_count_e(const E* __restrict__ x, int64_t n,
                                                       const uint32_t* __restrict__ state, u32x4* __restrict__ records,
                                                       int aligned) {
  constexpr int G = AqE<E>::G, NV = kAqChunk / (kAqBlock * G);
  __shared__ uint32_t s_c[2][kAqWaves];
  __shared__ double s_d[2][kAqWaves];
  const uint32_t cp = state[kAqCut], cn = state[kAqCut + 1];
  const int64_t c0 = (int64_t)blockIdx.x * kAqChunk;
  uint32_t ab = 0, ti = 0;                        // positive in the low half, negative in the high half
  double sp = 0.0, sn = 0.0;
#pragma unroll
  for (int j = 0; j < NV; ++j) {
    const int64_t e = c0 + (int64_t)(j * kAqBlock + threadIdx.x) * G;
    uint32_t u[G];
    aq_load<E>(x, e, n, aligned && e + G <= n, u);
#pragma unroll
    for (int i = 0; i < G; ++i) {
      const uint32_t m = u[i] & 0x7FFFFFFFu, s = u[i] >> 31, one = s ? 0x10000u : 1u;
      const uint32_t cut = s ? cn : cp;           // at least 1, so a zero is neither above nor at it
      const bool above = m > cut;
      const double v = (double)u2f(u[i]);
      ab += above ? one : 0u;
      ti += m == cut ? one : 0u;
      sp += above && !s ? v : 0.0;
      sn += above && s ? v : 0.0;
    }
  }
  ab = wave_sum(ab);
  ti = wave_sum(ti);
  sp = wave_sum(sp);
  sn = wave_sum(sn);
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  if (lane == 0) {
    s_c[0][w] = ab; s_c[1][w] = ti; s_d[0][w] = sp; s_d[1][w] = sn;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    ab = 0; ti = 0; sp = 0.0; sn = 0.0;
    for (int i = 0; i < kAqWaves; ++i) { ab += s_c[0][i]; ti += s_c[1][i]; sp += s_d[0][i]; sn += s_d[1][i]; }
    const uint64_t bp = (uint64_t)__double_as_longlong(sp), bn = (uint64_t)__double_as_longlong(sn);
    u32x4 r0, r1;
    r0[0] = ab & 0xFFFFu; r0[1] = ab >> 16; r0[2] = ti & 0xFFFFu; r0[3] = ti >> 16;
    r1[0] = (uint32_t)bp; r1[1] = (uint32_t)(bp >> 32); r1[2] = (uint32_t)bn; r1[3] = (uint32_t)(bn >> 32);
    records[2 * (int64_t)blockIdx.x] = r0;
    records[2 * (int64_t)blockIdx.x + 1] = r1;
  }
}

// ------------------------------------------------------------------------------------------------
// scan: one workgroup over the records in chunk order.  payload == nullptr (the world-1 step): only
// the tie bases and the means are produced.
__global__ __launch_bounds__(kAqSelBlock) void aq_scan(const u32x4* __restrict__ records, int64_t nchunks,
                                                       uint32_t* __restrict__ state, uint32_t* __restrict__ tbase,
                                                       uint8_t* __restrict__ payload, uint32_t cap) {
  __shared__ uint32_t s_w[kAqSelWaves + 1];
  __shared__ double s_d[2][kAqSelWaves];
  const uint32_t t = threadIdx.x, take_p = state[kAqTake], take_n = state[kAqTake + 1];
  uint32_t* dir = payload ? reinterpret_cast<uint32_t*>(payload + 16) : nullptr;
  uint32_t carry_p = 0, carry_n = 0, carry_e = 0;
  double dp = 0.0, dn = 0.0;                      // this thread's chunks, ascending
  for (int64_t base = 0; base < nchunks; base += kAqSelBlock) {
    const int64_t c = base + t;
    const bool live = c < nchunks;
    u32x4 r0 = {0u, 0u, 0u, 0u};
    if (live) {
      r0 = records[2 * c];
      const u32x4 r1 = records[2 * c + 1];
      dp += aq_f64(r1[0], r1[1]);
      dn += aq_f64(r1[2], r1[3]);
    }
    uint32_t tot;
    const uint32_t ep = block_excl_scan<kAqSelBlock>(r0[2], s_w, &tot) + carry_p;
    carry_p += tot;
    const uint32_t en = block_excl_scan<kAqSelBlock>(r0[3], s_w, &tot) + carry_n;
    carry_n += tot;
    const uint32_t gp = min(r0[2], take_p > ep ? take_p - ep : 0u), gn = min(r0[3], take_n > en ? take_n - en : 0u);
    const uint32_t sel = r0[0] + r0[1] + gp + gn;
    const uint32_t ee = block_excl_scan<kAqSelBlock>(sel, s_w, &tot) + carry_e;
    carry_e += tot;
    if (live) {
      tbase[2 * c] = ep;
      tbase[2 * c + 1] = en;
      if (dir) dir[c] = ee + sel;
    }
  }
  dp = wave_sum(dp);
  dn = wave_sum(dn);
  if ((t & 63u) == 0u) { s_d[0][t >> 6] = dp; s_d[1][t >> 6] = dn; }
  __syncthreads();
  if (t == 0) {
    dp = 0.0; dn = 0.0;
    for (int i = 0; i < kAqSelWaves; ++i) { dp += s_d[0][i]; dn += s_d[1][i]; }
    const uint32_t kp = state[kAqK], kn = state[kAqK + 1];
    if (kp) dp += (double)take_p * (double)u2f(state[kAqCut]);       // the ties taken all equal +-T
    if (kn) dn -= (double)take_n * (double)u2f(state[kAqCut + 1]);
    const float mp = kp ? (float)(dp / (double)kp) : 0.f, mn = kn ? (float)(dn / (double)kn) : 0.f;
    state[kAqMean] = f2u(mp);
    state[kAqMean + 1] = f2u(mn);
    if (payload) {
      u32x4 hdr;
      hdr[0] = f2u(mp); hdr[1] = f2u(mn); hdr[2] = carry_e; hdr[3] = cap;
      *reinterpret_cast<u32x4*>(payload) = hdr;
    }
  }
  if (!payload) return;
  // the directory's padding, the entries in [count, cap) and the entries' padding
  const int64_t dirw = (nchunks + 3) / 4 * 4;
  if (nchunks + t < dirw) dir[nchunks + t] = 0u;
  uint16_t* ent = reinterpret_cast<uint16_t*>(payload + 16 + 4 * dirw);
  const int64_t count = min(carry_e, cap), end = ((int64_t)cap + 7) & ~(int64_t)7;
  const int64_t a0 = min(end, (count + 7) & ~(int64_t)7);
  if (count + t < a0) ent[count + t] = 0;
  const u32x4 zero = {0u, 0u, 0u, 0u};
  for (int64_t v = a0 / 8 + t; v < end / 8; v += kAqSelBlock) reinterpret_cast<u32x4*>(ent)[v] = zero;
}

// ------------------------------------------------------------------------------------------------
// place: the chunk's flags as bit masks, the ties taken, then the entries in element order (or,
// STEP, the decoded chunk)
template <typename E, bool STEP>
__global__ __launch_bounds__(kAqBlock) void aq_place_e(const E* __restrict__ x, int64_t n, int64_t nchunks,
                                                       const uint32_t* __restrict__ state,
                                                       const uint32_t* __restrict__ tbase, uint8_t* __restrict__ payload,
                                                       uint32_t cap, E* __restrict__ out, int aligned, int aligned_out) {
  constexpr int G = AqE<E>::G, NV = kAqChunk / (kAqBlock * G), LPW = 32 / G;   // lanes a flag word
  __shared__ uint32_t sh_a[kAqWords], sh_t[kAqWords], sh_s[kAqWords];
  __shared__ uint32_t s_w[kAqWaves + 1];
  __shared__ u32x4 sh_stage[STEP ? 1 : kAqChunk / 8 + 1];
  const uint32_t t = threadIdx.x, cp = state[kAqCut], cn = state[kAqCut + 1];
  const uint32_t take_p = state[kAqTake], take_n = state[kAqTake + 1];
  const int64_t c = blockIdx.x, c0 = c * kAqChunk;
  const uint32_t sh = (t % LPW) * G;
#pragma unroll
  for (int j = 0; j < NV; ++j) {
    const uint32_t v = (uint32_t)j * kAqBlock + t;
    const int64_t e = c0 + (int64_t)v * G;
    uint32_t u[G];
    aq_load<E>(x, e, n, aligned && e + G <= n, u);
    uint32_t a = 0, ti = 0, sg = 0;
#pragma unroll
    for (int i = 0; i < G; ++i) {
      const uint32_t m = u[i] & 0x7FFFFFFFu, s = u[i] >> 31, cut = s ? cn : cp;
      a |= (m > cut ? 1u : 0u) << i;
      ti |= (m == cut ? 1u : 0u) << i;
      sg |= s << i;
    }
    a <<= sh; ti <<= sh; sg <<= sh;
#pragma unroll
    for (int o = 1; o < LPW; o <<= 1) {
      a |= __shfl_xor(a, o, 64);
      ti |= __shfl_xor(ti, o, 64);
      sg |= __shfl_xor(sg, o, 64);
    }
    if (t % LPW == 0) {
      sh_a[v / LPW] = a; sh_t[v / LPW] = ti; sh_s[v / LPW] = sg;
    }
  }
  __syncthreads();
  // one word a thread: elements 32 t .. 32 t + 31 of the chunk
  const uint32_t S = sh_s[t], tp = sh_t[t] & ~S, tn = sh_t[t] & S;
  const uint32_t ex = block_excl_scan<kAqBlock>((uint32_t)__popc(tp) | ((uint32_t)__popc(tn) << 16), s_w, nullptr);
  const uint32_t bp = tbase[2 * c] + (ex & 0xFFFFu), bn = tbase[2 * c + 1] + (ex >> 16);
  uint32_t sel = sh_a[t] | aq_first_bits(tp, take_p > bp ? take_p - bp : 0u) |
                 aq_first_bits(tn, take_n > bn ? take_n - bn : 0u);
  if constexpr (STEP) {
    sh_a[t] = sel;                                // its own word: nobody else read it
    __syncthreads();
    const float mp = u2f(state[kAqMean]), mn = u2f(state[kAqMean + 1]);
#pragma unroll
    for (int j = 0; j < NV; ++j) {
      const uint32_t v = (uint32_t)j * kAqBlock + t;
      const int64_t e = c0 + (int64_t)v * G;
      const uint32_t fs = sh_a[v / LPW] >> sh, fg = sh_s[v / LPW] >> sh;
      float d[G];
#pragma unroll
      for (int i = 0; i < G; ++i) d[i] = (fs >> i) & 1u ? ((fg >> i) & 1u ? mn : mp) : 0.f;
      aq_store<E>(out, e, n, aligned_out && e + G <= n, d);
    }
  } else {
    uint32_t total;
    const uint32_t pos = block_excl_scan<kAqBlock>((uint32_t)__popc(sel), s_w, &total);
    const uint32_t* dir = reinterpret_cast<const uint32_t*>(payload + 16);
    const int64_t g0 = c ? (int64_t)dir[c - 1] : 0, gb = g0 & ~(int64_t)7;
    uint16_t* stage = reinterpret_cast<uint16_t*>(sh_stage);
    uint32_t at = (uint32_t)(g0 - gb) + pos;      // staged at the destination's phase in its 16-byte line
    while (sel) {
      const uint32_t b = (uint32_t)__builtin_ctz(sel);
      sel &= sel - 1u;
      stage[at++] = (uint16_t)((((S >> b) & 1u) << 15) | (t * 32u + b));
    }
    __syncthreads();
    const int64_t dirw = (nchunks + 3) / 4 * 4;
    uint16_t* ent = reinterpret_cast<uint16_t*>(payload + 16 + 4 * dirw);
    const int64_t g1 = min(g0 + (int64_t)total, (int64_t)cap);
    const int64_t a0 = min(g1, (g0 + 7) & ~(int64_t)7), a1 = max(a0, g1 & ~(int64_t)7);
    if ((int64_t)t < a0 - g0) ent[g0 + t] = stage[g0 + t - gb];
    for (int64_t v = a0 / 8 + t; v < a1 / 8; v += kAqBlock) reinterpret_cast<u32x4*>(ent)[v] = sh_stage[v - gb / 8];
    if ((int64_t)t < g1 - a1) ent[a1 + t] = stage[a1 + t - gb];
  }
}

// ------------------------------------------------------------------------------------------------
// decode + aggregate
template <typename O>
__global__ __launch_bounds__(kAqBlock) void aq_decode_e(const uint8_t* __restrict__ payloads, int64_t stride, int world,
                                                        int64_t n, int64_t nchunks, uint32_t cap, float divisor,
                                                        O* __restrict__ out, int aligned) {
  constexpr int G = AqE<O>::G, NV = kAqChunk / (kAqBlock * G);
  __shared__ float sh_acc[kAqChunk];
  const uint32_t t = threadIdx.x;
  const int64_t c = blockIdx.x, c0 = c * kAqChunk;
  const uint32_t m = (uint32_t)min((int64_t)kAqChunk, n - c0);
  const int64_t ent_off = 16 + 4 * ((nchunks + 3) / 4 * 4);
  for (int i = t; i < kAqChunk; i += kAqBlock) sh_acc[i] = 0.f;
  __syncthreads();
  for (int w = 0; w < world; ++w) {
    const uint8_t* p = payloads + (int64_t)w * stride;
    const u32x4 hdr = *reinterpret_cast<const u32x4*>(p);
    if (hdr[3] == cap) {
      const uint32_t* dir = reinterpret_cast<const uint32_t*>(p + 16);
      const uint32_t lo = c ? dir[c - 1] : 0u, hi = dir[c], lim = min(hdr[2], cap);
      if (lo <= hi && hi <= lim) {
        const float mp = u2f(hdr[0]), mn = u2f(hdr[1]);
        const uint16_t* ent = reinterpret_cast<const uint16_t*>(p + ent_off);
        for (int64_t i = (int64_t)lo + t; i < (int64_t)hi; i += kAqBlock) {
          const uint32_t en = ent[i], off = en & (uint32_t)(kAqChunk - 1);
          if (off < m) sh_acc[off] = sh_acc[off] + (en >> 15 ? mn : mp);
        }
      }
    }
    __syncthreads();                              // rank order: the next rank adds to this one's sums
  }
#pragma unroll
  for (int j = 0; j < NV; ++j) {
    const uint32_t off = ((uint32_t)j * kAqBlock + t) * G;
    const int64_t e = c0 + off;
    float d[G];
#pragma unroll
    for (int i = 0; i < G; ++i) d[i] = divisor == 1.0f ? sh_acc[off + i] : sh_acc[off + i] / divisor;
    aq_store<O>(out, e, n, aligned && e + G <= n, d);
  }
}

// ------------------------------------------------------------------------------------------------
// host side: one typed launcher per f32 / bf16 pair
static inline bool aq_n_ok(int64_t n) { return n >= 0 && n < ((int64_t)1 << 31); }
static inline bool aq_ratio_ok(double r) { return r > 0.0 && r <= 1.0; }   // false for a NaN
static inline int64_t aq_cap(int64_t n, double r) { return (int64_t)__builtin_ceil((double)n * r) + 4; }
static inline size_t aq_payload(int64_t n, int64_t cap) { return (size_t)(16 + 4 * aq_dir_words(n) + 16 * ((cap + 7) / 8)); }
static inline size_t aq_workspace(int64_t n) {
  return al256(kAqOffRecords + (kAqRecordBytes + kAqTieBytes) * (size_t)aq_chunks(n));
}

// compress (out == nullptr) and the world-1 step (payload == nullptr)
template <typename E>
static grace_status_t aq_encode(const char* name, const char* bad, const E* x, int64_t n, double ratio, uint8_t* payload,
                                E* out, void* ws, size_t ws_bytes, void* stream) {
  GRACE_REQUIRE(x && (payload || out) && ws && aq_n_ok(n) && aq_ratio_ok(ratio) && AqE<E>::addressable(x) &&
                    AqE<E>::addressable(out) && al16(payload) && al16(ws) && ws_bytes >= aq_workspace(n),
                bad);
  if (n == 0) return GRACE_OK;
  constexpr int G = AqE<E>::G;
  constexpr int kLevels = sizeof(E) == 4 ? 3 : 2;  // bf16: 15 magnitude bits, 11 + 10 covers them
  const hipStream_t st = as_stream(stream);
  uint8_t* w = static_cast<uint8_t*>(ws);
  uint32_t* state = reinterpret_cast<uint32_t*>(w + kAqOffState);
  const int64_t nchunks = aq_chunks(n);
  u32x4* records = reinterpret_cast<u32x4*>(w + kAqOffRecords);
  uint32_t* tbase = reinterpret_cast<uint32_t*>(w + kAqOffRecords + kAqRecordBytes * (size_t)nchunks);
  const int al = al16(x) ? 1 : 0;
  const unsigned grid = stream_grid((n + G - 1) / G, kAqSelBlock, kAqSelGridCap);

  aq_zero<<<8, kAqSelBlock, 0, st>>>(reinterpret_cast<uint32_t*>(w), (int)(kAqOffRecords / sizeof(uint32_t)));
  GRACE_CHECK_LAUNCH(name);
  uint32_t* h0 = reinterpret_cast<uint32_t*>(w + kAqOffHist0);
  aq_hist_e<E><<<grid, kAqSelBlock, 0, st>>>(x, n, 20, 11, state, h0, al);
  GRACE_CHECK_LAUNCH(name);
  aq_resolve<kAqBins0><<<1, kAqSelBlock, 0, st>>>(h0, state, ratio, 11, 1, -1);
  GRACE_CHECK_LAUNCH(name);
  for (int l = 1; l < kLevels; ++l) {
    uint32_t* h = reinterpret_cast<uint32_t*>(w + (l == 1 ? kAqOffHist1 : kAqOffHist2));
    const int shift = 20 - 10 * l;
    aq_hist_e<E><<<grid, kAqSelBlock, 0, st>>>(x, n, shift, 10, state, h, al);
    GRACE_CHECK_LAUNCH(name);
    aq_resolve<kAqBins><<<1, kAqSelBlock, 0, st>>>(h, state, ratio, 10, 0, l == kLevels - 1 ? shift : -1);
    GRACE_CHECK_LAUNCH(name);
  }
  aq_count_e<E><<<(unsigned)nchunks, kAqBlock, 0, st>>>(x, n, state, records, al);
  GRACE_CHECK_LAUNCH(name);
  const uint32_t cap = (uint32_t)aq_cap(n, ratio);
  aq_scan<<<1, kAqSelBlock, 0, st>>>(records, nchunks, state, tbase, payload, cap);
  GRACE_CHECK_LAUNCH(name);
  if (payload)
    aq_place_e<E, false><<<(unsigned)nchunks, kAqBlock, 0, st>>>(x, n, nchunks, state, tbase, payload, cap, nullptr, al, 0);
  else
    aq_place_e<E, true><<<(unsigned)nchunks, kAqBlock, 0, st>>>(x, n, nchunks, state, tbase, nullptr, cap, out, al,
                                                                 al16(out) ? 1 : 0);
  GRACE_CHECK_LAUNCH(name);
  return GRACE_OK;
}

template <typename O>
static grace_status_t aq_decode(const char* name, const char* bad, const uint8_t* payloads, int64_t stride, int32_t world,
                                int64_t n, int64_t cap, float divisor, O* out, void* stream) {
  GRACE_REQUIRE(payloads && out && world >= 1 && world <= 1024 && aq_n_ok(n) && cap >= 0 && cap <= n + 4 &&
                    divisor != 0.0f && stride >= 0 && stride % 16 == 0 && (n == 0 || stride >= (int64_t)aq_payload(n, cap)) &&
                    al16(payloads) && AqE<O>::addressable(out),
                bad);
  if (n == 0) return GRACE_OK;
  aq_decode_e<O><<<(unsigned)aq_chunks(n), kAqBlock, 0, as_stream(stream)>>>(payloads, stride, world, n, aq_chunks(n),
                                                                            (uint32_t)cap, divisor, out, al16(out) ? 1 : 0);
  GRACE_CHECK_LAUNCH(name);
  return GRACE_OK;
}

}  // namespace grace

using namespace grace;

extern "C" {

int64_t grace_adaq_capacity(int64_t n, double ratio) {
  return n > 0 && aq_n_ok(n) && aq_ratio_ok(ratio) ? aq_cap(n, ratio) : 0;
}

size_t grace_adaq_payload_bytes(int64_t n, double ratio) {
  return n > 0 && aq_n_ok(n) && aq_ratio_ok(ratio) ? aq_payload(n, aq_cap(n, ratio)) : 0;
}

size_t grace_adaq_workspace_bytes(int64_t n) { return aq_n_ok(n) ? aq_workspace(n) : 0; }

grace_status_t grace_adaq_compress(const float* x, int64_t n, double ratio, uint8_t* payload, void* ws, size_t ws_bytes,
                                   void* stream) {
  GRACE_REQUIRE(payload, "grace_adaq_compress: bad arguments");
  return aq_encode<float>("grace_adaq_compress", "grace_adaq_compress: bad arguments", x, n, ratio, payload, nullptr, ws,
                          ws_bytes, stream);
}

grace_status_t grace_adaq_compress_bf16(const uint16_t* x, int64_t n, double ratio, uint8_t* payload, void* ws,
                                        size_t ws_bytes, void* stream) {
  GRACE_REQUIRE(payload, "grace_adaq_compress_bf16: bad arguments");
  return aq_encode<uint16_t>("grace_adaq_compress_bf16", "grace_adaq_compress_bf16: bad arguments", x, n, ratio, payload,
                             nullptr, ws, ws_bytes, stream);
}

grace_status_t grace_adaq_step_w1(const float* x, int64_t n, double ratio, float* out, void* ws, size_t ws_bytes,
                                  void* stream) {
  GRACE_REQUIRE(out, "grace_adaq_step_w1: bad arguments");
  return aq_encode<float>("grace_adaq_step_w1", "grace_adaq_step_w1: bad arguments", x, n, ratio, nullptr, out, ws,
                          ws_bytes, stream);
}

grace_status_t grace_adaq_step_w1_bf16(const uint16_t* x, int64_t n, double ratio, uint16_t* out, void* ws,
                                       size_t ws_bytes, void* stream) {
  GRACE_REQUIRE(out, "grace_adaq_step_w1_bf16: bad arguments");
  return aq_encode<uint16_t>("grace_adaq_step_w1_bf16", "grace_adaq_step_w1_bf16: bad arguments", x, n, ratio, nullptr,
                             out, ws, ws_bytes, stream);
}

grace_status_t grace_adaq_decode_aggregate(const uint8_t* payloads, int64_t stride_bytes, int32_t world, int64_t n,
                                           int64_t cap, float divisor, float* out, void* stream) {
  return aq_decode<float>("grace_adaq_decode_aggregate", "grace_adaq_decode_aggregate: bad arguments", payloads,
                          stride_bytes, world, n, cap, divisor, out, stream);
}

grace_status_t grace_adaq_decode_aggregate_bf16(const uint8_t* payloads, int64_t stride_bytes, int32_t world,
                                                int64_t n, int64_t cap, float divisor, uint16_t* out, void* stream) {
  return aq_decode<uint16_t>("grace_adaq_decode_aggregate_bf16", "grace_adaq_decode_aggregate_bf16: bad arguments",
                             payloads, stride_bytes, world, n, cap, divisor, out, stream);
}

}  // extern "C"
