// Rank-ordered aggregate of capacity-bounded exchange records as a bfloat16 dense result (the
// world > 1 decode of Allgather(DgcCompressor) on a bfloat16 gradient), and of the
// padded buffers of the threshold counts exchange (grace_sparse_aggregate_padded_bf16):
// the same two kernels, told where a rank's count, values and indices are by a RecSrc.
//
// The f32 decode of sparse.hip (grace_sparse_aggregate_capped) fills the n-element output, scatters
// one rank per launch with an n-element tag array beside it, and divides in a last launch; a bf16
// user narrowed that on top (4n + 2n bytes more).  The records' indices ascend within a rank (the
// torch.where order dgc_write_kernel and thr_write_kernel produce), so the output can be decoded tile
// by tile as payload.hip decodes its grouped payloads: a workgroup owns an 8192-element chunk, adds
// every rank's entries of that chunk into an f32 LDS tile rank by rank -- ((0 + d0) + d1) + ...
// exactly as Python's sum, since indices are unique within a rank and a barrier separates the ranks
// -- divides once, rounds once (common.h f32_to_bf16) and stores 16 B per lane: 2 B per element
// written, zeros included, in one launch with no fill, no tags and no sort.
//
// Where rank w's entries of chunk c begin and end comes from a streaming boundary pass over the
// index arrays (one launch before the decode): the thread at position p writes p as the begin of
// every chunk in (chunk(idx[p - 1]), chunk(idx[p])], with chunk(idx[-1]) = -1 and chunk(idx[count])
// = the chunk count, so every one of the nchunks + 1 boundaries of a rank is written whatever the
// counts are (a rank with no entries: one thread writes them all).  (A/B against a binary search per
// workgroup in front of the tile, lane w searching rank w's indices, no boundary pass: 2^26 elements,
// W = 8, 5.5 M entries, 81.2 us with the pass against 155.8; at n = 50,000, launch bound, 13.9 against
// 10.8 -- profiles/dgc_bf16_bench.txt.)  Both kernels are memory-safe
// for any record contents: a boundary is a position in [0, count], an index outside [0, n) or
// outside the chunk it was filed under is skipped, and positions past min(count, cap) are not read.
#include "common.h"
#include "../../include/grace_hip_dgc.h"
#include "../../include/grace_hip_sparse.h"

namespace grace {

constexpr int kRChunkLog = 13;
constexpr int kRChunk = 1 << kRChunkLog;   // output elements per workgroup: a 32 KB f32 tile
constexpr int kRBlock = 256;               // payload.hip's decode workgroup (its A/B: 256 threads won)
constexpr int kRHdr = 4;                   // = sparse.hip kRecHdr (grace_exchange_record_words)
constexpr int kRMaxRanks = 1024;           // = payload.hip kMaxRanks, the sorted decode's limit
constexpr int kRBatch = 8;                 // ranks whose entry loads are in flight together
constexpr int kRLane = 8;                  // bf16 results per lane per store: 16 B

// Where rank w's count, values and indices are: the capacity-bounded records ({count, cap, 0, 0 | vals
// f32[cap] | idx i32[cap]}, hdr = 4, counts null: the count is the header's first word), or the padded
// buffers of the threshold counts exchange ({vals f32[cap] | idx i32[cap]}, hdr = 0, the counts in a
// device int32[world] array beside them; grace_sparse_aggregate_padded_bf16).  Both kernels below
// read a rank through this and nothing else.
struct RecSrc {
  const uint32_t* base;
  int64_t stride;          // words between two ranks
  int64_t cap;
  const int32_t* counts;   // null: the record header holds the count
  int hdr;                 // header words in front of vals
  __device__ __forceinline__ int64_t count(int w) const {   // entries that may be read: in [0, cap]
    const int64_t c = counts ? (int64_t)max(counts[w], 0) : (int64_t)base[(int64_t)w * stride];
    return min(c, cap);
  }
  __device__ __forceinline__ const float* vals(int w) const {
    return reinterpret_cast<const float*>(base + (int64_t)w * stride + hdr);
  }
  __device__ __forceinline__ const int32_t* idx(int w) const {
    return reinterpret_cast<const int32_t*>(base + (int64_t)w * stride + hdr + cap);
  }
};

__device__ __forceinline__ int rec_chunk_of(int32_t i, int nchunks) {
  const uint32_t c = (uint32_t)i >> kRChunkLog;   // a negative index lands past every chunk
  return c < (uint32_t)nchunks ? (int)c : nchunks;
}

// bounds[w][c] = the first position of rank w whose index is in chunk c or later, c in [0, nchunks]
__global__ __launch_bounds__(kRBlock) void rec_bounds_kernel(RecSrc src, int nchunks, int32_t* __restrict__ bounds) {
  const int64_t cnt = src.count(blockIdx.y);
  const int32_t* __restrict__ idx = src.idx(blockIdx.y);
  int32_t* bw = bounds + (int64_t)blockIdx.y * (nchunks + 1);
  for (int64_t p = (int64_t)blockIdx.x * kRBlock + threadIdx.x; p <= cnt; p += (int64_t)gridDim.x * kRBlock) {
    const int lo = p == 0 ? -1 : rec_chunk_of(idx[p - 1], nchunks);
    const int hi = p == cnt ? nchunks : rec_chunk_of(idx[p], nchunks);
    for (int c = lo + 1; c <= hi; ++c) bw[c] = (int32_t)p;
  }
}

// SMALLW (world <= 64): lane w of every wave keeps rank w's two boundaries in registers, so the tile
// is the workgroup's only LDS (payload.hip chunk_accumulate_kernel's arrangement: 32 KB, five
// workgroups per CU instead of four with the 8 KB table beside it).
template <bool SMALLW>
__global__ __launch_bounds__(kRBlock) void rec_accumulate_bf16_kernel(RecSrc src, const int32_t* __restrict__ bounds,
                                                                     int nchunks, int world, float divisor,
                                                                     uint16_t* __restrict__ out, int64_t n,
                                                                     uint32_t* __restrict__ stat) {
  __shared__ float tile[kRChunk];
  __shared__ int32_t s_b[SMALLW ? 1 : 2 * kRMaxRanks];
  const int t = threadIdx.x;
  const int ch = blockIdx.x;
  const int64_t c0 = (int64_t)ch << kRChunkLog;
  int32_t bl = 0, el = 0;   // SMALLW: lane w's rank-w boundaries
  if constexpr (SMALLW) {
    const int lane = t & 63;
    if (lane < world) {
      const int32_t* bw = bounds + (int64_t)lane * (nchunks + 1);
      bl = bw[ch];
      el = bw[ch + 1];
    }
  } else {
    for (int w = t; w < world; w += kRBlock) {
      const int32_t* bw = bounds + (int64_t)w * (nchunks + 1);
      s_b[2 * w] = bw[ch];
      s_b[2 * w + 1] = bw[ch + 1];
    }
  }
  auto bnd = [&](int w, int32_t& b, int32_t& e) {   // w wave-uniform
    if constexpr (SMALLW) {
      b = __builtin_amdgcn_readlane(bl, w);
      e = __builtin_amdgcn_readlane(el, w);
    } else {
      b = s_b[2 * w];
      e = s_b[2 * w + 1];
    }
  };
  // the entry at position p of rank w as its offset inside this chunk, or -1 if it is not one of it
  auto local = [&](int32_t i) -> int32_t {
    const int64_t li = (int64_t)i - c0;
    return (li >= 0 && li < kRChunk && (int64_t)i < n) ? (int32_t)li : -1;
  };
  if (stat && ch == 0 && t == 0) {   // grace_sparse_aggregate_capped's stat (records only), identical on every rank
    uint32_t mx = 0u;
    for (int w = 0; w < world; ++w) mx = max(mx, src.base[(int64_t)w * src.stride]);
    stat[0] = mx;
    stat[1] = (int64_t)mx > src.cap ? 1u : 0u;
  }
  for (int e = t; e < kRChunk; e += kRBlock) tile[e] = 0.f;
  __syncthreads();
  for (int w0 = 0; w0 < world; w0 += kRBatch) {
    int32_t l[kRBatch];
    float v[kRBatch];
#pragma unroll
    for (int q = 0; q < kRBatch; ++q) {   // unconditional (clamped) loads: all in flight at once
      const int w = w0 + q < world ? w0 + q : w0;
      int32_t b, e;
      bnd(w, b, e);
      const int64_t p = (int64_t)b + t;   // 64-bit: b + t may pass 2^31
      const bool ok = w0 + q < world && p < e;
      v[q] = src.vals(w)[ok ? p : 0];   // position 0 exists (cap >= 1), its value unused
      const int32_t i = src.idx(w)[ok ? p : 0];
      l[q] = ok ? local(i) : -1;
    }
#pragma unroll
    for (int q = 0; q < kRBatch; ++q) {
      const int w = w0 + q;
      if (w >= world) break;
      if (l[q] >= 0) tile[l[q]] = tile[l[q]] + v[q];
      int32_t s0, s1;
      bnd(w, s0, s1);
      // a rank with more than a block-width of entries here finishes its rounds before the next rank
      // (indices are unique within a rank, so its own rounds need no barrier between them)
      const float* __restrict__ wv = src.vals(w);
      const int32_t* __restrict__ wi = src.idx(w);
      for (int64_t p = (int64_t)s0 + kRBlock + t; p < s1; p += kRBlock) {
        const int32_t lp = local(wi[p]);
        if (lp >= 0) tile[lp] = tile[lp] + wv[p];
      }
      __syncthreads();
    }
  }
  // the sum is divided in f32 and rounded once (common.h f32_to_bf16, not the hardware convert)
  typedef uint32_t uv __attribute__((ext_vector_type(kRLane / 2)));
  if (c0 + kRChunk <= n && (reinterpret_cast<uintptr_t>(out) & (2u * kRLane - 1u)) == 0) {
    for (int e = t * kRLane; e < kRChunk; e += kRBlock * kRLane) {
      uv p;
#pragma unroll
      for (int j = 0; j < kRLane / 2; ++j) {
        float a = tile[e + 2 * j], b = tile[e + 2 * j + 1];
        if (divisor != 1.0f) { a = a / divisor; b = b / divisor; }
        p[j] = pack_bf16x2(a, b);
      }
      __builtin_nontemporal_store(p, reinterpret_cast<uv*>(out + c0 + e));
    }
  } else {
    for (int e = t; e < kRChunk && c0 + e < n; e += kRBlock)
      out[c0 + e] = f32_to_bf16(divisor != 1.0f ? tile[e] / divisor : tile[e]);
  }
}

static size_t rec_bounds_bytes(int32_t world, int64_t n) {
  const int64_t nchunks = (n + kRChunk - 1) / kRChunk;
  return ((sizeof(int32_t) * (size_t)world * (size_t)(nchunks + 1)) + 255) & ~(size_t)255;
}

}  // namespace grace

using namespace grace;

extern "C" {

size_t grace_sparse_aggregate_records_bf16_workspace_bytes(int32_t world, int64_t n) {
  if (world < 1 || world > kRMaxRanks || n < 1 || n >= ((int64_t)1 << 31)) return 0;
  return rec_bounds_bytes(world, n);
}

// the boundary pass and the tile decode over either layout
static grace_status_t rec_decode_bf16(const char* name, const RecSrc& src, int32_t world, float divisor, uint16_t* out,
                                      int64_t n, uint32_t* stat, void* ws, hipStream_t s) {
  const int nchunks = (int)((n + kRChunk - 1) / kRChunk);
  int32_t* bounds = reinterpret_cast<int32_t*>(ws);
  rec_bounds_kernel<<<dim3(stream_grid(src.cap + 1, kRBlock, 1024), (unsigned)world), kRBlock, 0, s>>>(src, nchunks,
                                                                                                     bounds);
  GRACE_CHECK_LAUNCH(name);
  if (world <= kWave)
    rec_accumulate_bf16_kernel<true><<<(unsigned)nchunks, kRBlock, 0, s>>>(src, bounds, nchunks, world, divisor, out, n,
                                                                          stat);
  else
    rec_accumulate_bf16_kernel<false><<<(unsigned)nchunks, kRBlock, 0, s>>>(src, bounds, nchunks, world, divisor, out, n,
                                                                           stat);
  GRACE_CHECK_LAUNCH(name);
  return GRACE_OK;
}

grace_status_t grace_sparse_aggregate_records_bf16(const uint32_t* recs, int64_t stride, int64_t cap, int32_t world,
                                                   float divisor, uint16_t* out, int64_t n, uint32_t* stat, void* ws,
                                                   size_t ws_bytes, void* stream) {
  GRACE_REQUIRE(recs && out && stat && ws && world >= 1 && world <= kRMaxRanks && cap >= 1 && cap <= n &&
                    n < ((int64_t)1 << 31) && stride == kRHdr + 2 * cap,
                "grace_sparse_aggregate_records_bf16: bad arguments (1 <= cap <= n < 2^31, 1 <= world <= 1024, "
                "stride = 4 + 2 cap)");
  GRACE_REQUIRE(ws_bytes >= rec_bounds_bytes(world, n), "grace_sparse_aggregate_records_bf16: workspace too small");
  return rec_decode_bf16("grace_sparse_aggregate_records_bf16", RecSrc{recs, stride, cap, nullptr, kRHdr}, world, divisor,
                         out, n, stat, ws, as_stream(stream));
}

size_t grace_sparse_aggregate_padded_bf16_workspace_bytes(int32_t world, int64_t n) {
  return grace_sparse_aggregate_records_bf16_workspace_bytes(world, n);
}

grace_status_t grace_sparse_aggregate_padded_bf16(const uint32_t* base, int64_t cap, const int32_t* counts,
                                                  int32_t world, float divisor, uint16_t* out, int64_t n, void* ws,
                                                  size_t ws_bytes, void* stream) {
  GRACE_REQUIRE(base && counts && out && ws && world >= 1 && world <= kRMaxRanks && cap >= 1 && cap <= n &&
                    n < ((int64_t)1 << 31),
                "grace_sparse_aggregate_padded_bf16: bad arguments (1 <= cap <= n < 2^31, 1 <= world <= 1024)");
  GRACE_REQUIRE(ws_bytes >= rec_bounds_bytes(world, n), "grace_sparse_aggregate_padded_bf16: workspace too small");
  return rec_decode_bf16("grace_sparse_aggregate_padded_bf16", RecSrc{base, 2 * cap, cap, counts, 0}, world, divisor, out,
                         n, nullptr, ws, as_stream(stream));
}

}  // extern "C"
