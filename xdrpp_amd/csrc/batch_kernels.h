// What the RPC batch stages share (verify_kernels.h, replies_kernels.h,
// reply_batch_kernels.h, call_batch_kernels.h, pending_kernels.h).  Every stage
// is count -> scan -> emit over 256-item tiles:
//
//   tile_reduce    a workgroup's 256 lanes to one sum and one count per tile
//   k_tile_scan    exclusive scan of the tile words in one workgroup of 1024,
//                  1024 tiles a round with the carry of the rounds before; the
//                  totals go to an epilogue (gather_totals, stream_totals,
//                  count_total)
//   sources        what xdrg_encode wrote for one result type or procedure and
//                  the message each entry belongs to (xdrg_rpc_result_src,
//                  xdrg_rpc_arg_src): k_owner_fill, then k_src_claim, one lane
//                  per entry, every source in one launch -- a usable entry
//                  claims its message with a 64-bit atomicMin of
//                  (source << 32 | position), so the lowest entry wins
//                  whatever the order the lanes run in
//   stretch emit   the items of a wave's 64 lanes are one contiguous stretch of
//                  the output: stretch_place gives each its offset and the
//                  wave its 64 byte ends in LDS, stretch_write copies the
//                  stretch with consecutive lanes on consecutive words (W = 4)
//                  or aligned 16-byte chunks (W = 16), each word's message
//                  found by a binary search of the ends (stretch_find)
//
// The kernels are templates, so every translation unit that launches one
// links its own instance.
#pragma once
#include <hip/hip_runtime.h>

#include "dev_common.h"

namespace xdrg {
namespace dev {

constexpr uint32_t kTileThreads = 256;   // items a tile
constexpr uint32_t kScanThreads = 1024;  // tiles a round of the scan

// ------------------------------------------------------------------ tiles
// tile_sum[blockIdx.x] = the workgroup's sum of v (nullptr: no sum),
// tile_cnt[blockIdx.x] = its lanes with `flag`.  Every lane of the
// kTileThreads must call.
__device__ __forceinline__ void tile_reduce(unsigned long long v, bool flag, unsigned long long *__restrict__ tile_sum,
                                            unsigned long long *__restrict__ tile_cnt) {
  __shared__ unsigned long long ws[kTileThreads / 64];
  __shared__ uint32_t wc[kTileThreads / 64];
  const unsigned long long m = __ballot(flag);
  if (tile_sum)
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  if ((threadIdx.x & 63u) == 0u) {
    if (tile_sum) ws[threadIdx.x >> 6] = v;
    wc[threadIdx.x >> 6] = __popcll(m);
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    unsigned long long ss = 0, sc = 0;
    for (uint32_t k = 0; k < kTileThreads / 64; ++k) {
      if (tile_sum) ss += ws[k];
      sc += wc[k];
    }
    if (tile_sum) tile_sum[blockIdx.x] = ss;
    tile_cnt[blockIdx.x] = sc;
  }
}

// The totals of COLS tile columns of nb words each to epi(totals, lane), run
// by the first wave (all 64 lanes); the first SCANNED columns are replaced by
// their exclusive scans.  One workgroup; nb == 0 reads and writes no tile.
template <int SCANNED, int COLS, class EPI>
__global__ __launch_bounds__(kScanThreads) void k_tile_scan(unsigned long long *__restrict__ tile_a,
                                                            unsigned long long *__restrict__ tile_b, uint64_t nb,
                                                            const EPI epi) {
  static_assert(1 <= SCANNED && SCANNED <= COLS && COLS <= 2, "one or two columns");
  __shared__ unsigned long long ws[COLS][kScanThreads / 64];
  unsigned long long *const tile[2] = {tile_a, tile_b};
  const uint32_t tid = threadIdx.x, lane = tid & 63u, wid = tid >> 6;
  unsigned long long carry[COLS] = {};
  for (uint64_t t0 = 0; t0 < nb; t0 += kScanThreads) {
    const uint64_t j = t0 + tid;
    unsigned long long v[COLS], iv[COLS];
#pragma unroll
    for (int c = 0; c < COLS; ++c) {
      v[c] = j < nb ? tile[c][j] : 0ull;
      iv[c] = wave_incl_scan64(v[c]);
      if (lane == 63u) ws[c][wid] = iv[c];
    }
    __syncthreads();
#pragma unroll
    for (int c = 0; c < COLS; ++c) {
      unsigned long long base = carry[c], total = 0;
      for (uint32_t k = 0; k < kScanThreads / 64; ++k) {
        if (k < wid) base += ws[c][k];
        total += ws[c][k];
      }
      if (c < SCANNED && j < nb) tile[c][j] = base + iv[c] - v[c];
      carry[c] += total;
    }
    __syncthreads();  // ws reused by the next round
  }
  if (wid == 0) epi(carry, lane);
}

// ---------------------------------------------------------------- sources
static_assert(XDRG_RPC_MAX_RESULT_SRCS == XDRG_RPC_MAX_ARG_SRCS, "one source table serves both");
constexpr uint32_t kMaxSrcs = XDRG_RPC_MAX_RESULT_SRCS;
constexpr unsigned long long kNoOwner = ~0ull;

// What the claim needs of a source.  A source without bytes (d_bytes NULL)
// arrives with offsets = nullptr and fixed = 0: every span is [0, 0).
struct src_claim {
  const uint64_t *index;
  const uint64_t *count;    // nullptr: cap entries
  const uint64_t *offsets;  // nullptr: fixed-size entries
  uint64_t bytes_len;
  uint32_t cap, fixed;
};
struct src_claim_table {
  src_claim e[kMaxSrcs];
  uint32_t blk[kMaxSrcs + 1];  // first workgroup of each source
};
// The counts alone, for the kernels that sum the entries.
struct src_count_table {
  const uint64_t *count[kMaxSrcs];
  uint32_t cap[kMaxSrcs];
};
static_assert(sizeof(src_claim_table) < 4096 && sizeof(src_count_table) + 64 < 4096, "kernel arguments under 4 KiB");

__device__ __forceinline__ uint64_t src_count(const uint64_t *count, uint32_t cap) {
  const uint64_t c = count ? *count : cap;
  return c < cap ? c : cap;
}

// The entries of every source (lanes 0..63 of the calling wave, all active).
__device__ __forceinline__ unsigned long long src_entries(const src_count_table &T, uint32_t nsrcs, uint32_t lane) {
  unsigned long long c = 0;
  for (uint32_t k = 0; k < nsrcs; ++k)  // uniform k: the table is read with scalar loads
    if (lane == k) c = src_count(T.count[k], T.cap[k]);
  for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o, 64);
  return c;
}

// Bytes [*a, *b) of entry `pos` of a source (any struct with offsets and fixed).
template <class S>
__device__ __forceinline__ void src_span(const S &s, uint64_t pos, uint64_t *a, uint64_t *b) {
  *a = s.offsets ? s.offsets[pos] : pos * s.fixed;
  *b = s.offsets ? s.offsets[pos + 1] : *a + s.fixed;
}

// An owner word's source and entry.
__device__ __forceinline__ uint32_t owner_src(unsigned long long own) {
  return static_cast<uint32_t>(own >> 32) & (kMaxSrcs - 1u);
}
__device__ __forceinline__ uint64_t owner_pos(unsigned long long own) { return own & 0xffffffffull; }

// (k_owner_fill and k_src_count_entries take no template argument of their
// own: templates only so that they link like the rest.)
template <class = void>
__global__ __launch_bounds__(kTileThreads) void k_owner_fill(unsigned long long *__restrict__ owner, uint64_t n) {
  const uint64_t i = static_cast<uint64_t>(blockIdx.x) * kTileThreads + threadIdx.x;
  if (i < n) owner[i] = kNoOwner;
}

// n == 0: no message is left without an entry, every entry is unused.
template <class = void>
__global__ __launch_bounds__(64) void k_src_count_entries(const src_count_table T, uint32_t nsrcs,
                                                          unsigned long long *__restrict__ unsent,
                                                          unsigned long long *__restrict__ unused) {
  const unsigned long long c = src_entries(T, nsrcs, threadIdx.x);
  if (threadIdx.x == 0) {
    if (unsent) *unsent = 0;
    *unused = c;
  }
}

// One lane per entry.  The workgroup's source is found by a uniform loop over
// the table (kernel arguments: scalar loads).  USABLE: usable(i), whether
// message i takes an entry at all, and kHdrBytes, what a message holds besides
// the entry's bytes (they count against XDRG_MAX_MSG).
template <class USABLE>
__global__ __launch_bounds__(kTileThreads) void k_src_claim(uint64_t n, const src_claim_table T, uint32_t nsrcs,
                                                            const USABLE usable,
                                                            unsigned long long *__restrict__ owner) {
  uint32_t s = 0;
  for (uint32_t k = 1; k < nsrcs; ++k) s = T.blk[k] <= blockIdx.x ? k : s;
  const src_claim S = T.e[s];
  const uint64_t pos = static_cast<uint64_t>(blockIdx.x - T.blk[s]) * kTileThreads + threadIdx.x;
  if (pos >= src_count(S.count, S.cap)) return;
  const uint64_t i = S.index[pos];
  if (i < n && usable(i)) {
    uint64_t a, b;
    src_span(S, pos, &a, &b);
    if (b >= a && b <= S.bytes_len && !((a | b) & 3u) && b - a <= XDRG_MAX_MSG - USABLE::kHdrBytes)
      atomicMin(owner + i, (static_cast<unsigned long long>(s) << 32) | pos);
  }
}

// ----------------------------------------------------------- scan epilogues
// A gather: the selected items to *count, their bytes to offsets[count] and
// status->total_bytes.
struct gather_totals {
  uint64_t *count, *offsets;
  xdrg_status *status;
  __device__ void operator()(const unsigned long long (&t)[2], uint32_t lane) const {
    if (lane) return;
    *count = t[0];
    offsets[t[0]] = t[1];
    status->total_bytes = t[1];
  }
};

// A message stream built from sources: t[0] its bytes, to *total_at and
// status->total_bytes, t[1] the messages an entry won; *unsent = the messages
// no entry won, *unused = the entries of every source less the winners (tile
// sums, no atomic on one word: DESIGN.md 7.2.3).  Either may be nullptr.
struct stream_totals {
  src_count_table T;
  uint32_t nsrcs;
  uint64_t n;
  uint64_t *total_at;
  xdrg_status *status;
  unsigned long long *unsent, *unused;
  __device__ void operator()(const unsigned long long (&t)[2], uint32_t lane) const {
    const unsigned long long entries = unused ? src_entries(T, nsrcs, lane) : 0ull;
    if (lane) return;
    *total_at = t[0];
    status->total_bytes = t[0];
    if (unsent) *unsent = n - t[1];
    if (unused) *unused = entries - t[1];
  }
};

// A compaction: the kept items to *count.
struct count_total {
  uint64_t *count;
  __device__ void operator()(const unsigned long long (&t)[1], uint32_t lane) const {
    if (lane == 0) *count = t[0];
  }
};

// ------------------------------------------------------------ stretch emit
// Where this lane's `bytes` go (at): the tile's base, the waves before this
// one (wbase: where the wave's stretch starts) and the lanes before this one.
// An item that is `present` and does not fit the capacity is
// XDRG_ERR_OVERFLOW_PUT at item i (nothing of it is written, nor of the ones
// after it): end[lane] = the wave's byte ends of the items that fit, a prefix
// of its stretch.  put(at) is the caller's store of the offset, called before
// the checks: the caller's __syncthreads(), which publishes `end`, waits for
// the wave's global stores, and an early one has the checks to complete in.
// The barrier in here orders whatever the caller wrote to LDS before.
struct stretch_at {
  uint64_t at, wbase;
  bool fits;
};
template <class PUT>
__device__ __forceinline__ stretch_at stretch_place(uint64_t bytes, bool present, uint64_t i,
                                                    const unsigned long long *__restrict__ tile_bytes, uint64_t cap,
                                                    unsigned long long *err, unsigned long long *end, PUT &&put) {
  __shared__ unsigned long long wb[kTileThreads / 64];
  const uint32_t lane = threadIdx.x & 63u, wid = threadIdx.x >> 6;
  const uint64_t ib = wave_incl_scan64(bytes);
  if (lane == 63u) wb[wid] = ib;
  __syncthreads();
  stretch_at p{0, tile_bytes[blockIdx.x], false};
  for (uint32_t k = 0; k < wid; ++k) p.wbase += wb[k];
  p.at = p.wbase + ib - bytes;
  put(p.at);
  if (present) {
    p.fits = p.at <= cap && bytes <= cap - p.at;
    if (!p.fits) report(err, i, kOpRecordLevel, XDRG_ERR_OVERFLOW_PUT);  // xdr_generic_put::check (marshal.h:104-108)
  }
  end[lane] = wave_incl_scan64(p.fits ? bytes : 0u);
  return p;
}

// The first item of the wave whose end is past `off` (off < end[63]).
__device__ __forceinline__ uint32_t stretch_find(const unsigned long long *end, uint64_t off) {
  uint32_t lo = 0, hi = 63;
  while (lo < hi) {
    const uint32_t mid = (lo + hi) >> 1;
    if (end[mid] > off) hi = mid; else lo = mid + 1;
  }
  return lo;
}

// A wave's LDS: byte ends and payload pointers of its 64 messages and the
// words each message starts with (HDR_WORDS x 64, one column per message: a
// lane writes its column without bank conflicts).  VAR_NW: message m starts
// with nw[m] of them, else with all.  A message with a payload starts with
// PAYLOAD_AT words, and src[m] holds the rest.
template <uint32_t HDR_WORDS, bool VAR_NW, uint32_t PAYLOAD_AT = HDR_WORDS>
struct wave_stretch {
  static constexpr uint32_t kPayloadAt = PAYLOAD_AT;
  unsigned long long end[64];
  const uint8_t *src[64];
  uint32_t w[HDR_WORDS][64];
  __device__ __forceinline__ uint32_t words(uint32_t) const { return HDR_WORDS; }
};
template <uint32_t HDR_WORDS, uint32_t PAYLOAD_AT>
struct wave_stretch<HDR_WORDS, true, PAYLOAD_AT> : wave_stretch<HDR_WORDS, false, PAYLOAD_AT> {
  uint32_t nw[64];
  __device__ __forceinline__ uint32_t words(uint32_t m) const { return nw[m]; }
};

// Word `k` of message `m` of the wave.
template <class L>
__device__ __forceinline__ uint32_t stretch_word(const L &lds, uint32_t m, uint64_t k) {
  return k < lds.words(m) ? lds.w[k][m] : ld32(lds.src[m] + 4u * (k - L::kPayloadAt));
}

// The wave's stretch to `base`, W bytes a lane per step.  Everything is whole
// aligned words (the claim refuses entries that are not), so there is no byte
// path.
template <int W, class L>
__device__ __forceinline__ void stretch_write(const L &lds, uint8_t *__restrict__ base, uint32_t lane) {
  const uint64_t total = lds.end[63];
  if constexpr (W == 4) {
    for (uint64_t off = 4ull * lane; off < total; off += 256u) {
      const uint32_t m = stretch_find(lds.end, off);
      const uint64_t start = m ? lds.end[m - 1] : 0u;
      st32(base + off, stretch_word(lds, m, (off - start) >> 2));
    }
  } else {
    // Aligned 16-byte chunks of the output: chunk c holds the stretch's bytes
    // [16 c - pre, 16 c - pre + 16), the first and the last may be partial.
    const uint64_t pre = reinterpret_cast<uintptr_t>(base) & 15u;
    const uint64_t nchunks = total ? (pre + total + 15u) >> 4 : 0u;
    for (uint64_t c = lane; c < nchunks; c += 64u) {
      const int64_t o0 = static_cast<int64_t>(16u * c) - static_cast<int64_t>(pre);
      const bool full = o0 >= 0 && static_cast<uint64_t>(o0) + 16u <= total;
      const uint64_t first = o0 < 0 ? 0u : static_cast<uint64_t>(o0);
      uint32_t m = stretch_find(lds.end, first);
      const uint64_t start = m ? lds.end[m - 1] : 0u, k0 = (first - start) >> 2;
      if (full && k0 >= lds.words(m) && first + 16u <= lds.end[m]) {  // four words of one payload
        *reinterpret_cast<u32x4 *>(base + o0) = ld16u(lds.src[m] + 4u * (k0 - L::kPayloadAt));
        continue;
      }
      uint32_t v[4] = {0u, 0u, 0u, 0u};
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int64_t oj = o0 + 4 * j;
        if (oj < 0 || static_cast<uint64_t>(oj) >= total) continue;
        const uint64_t o = static_cast<uint64_t>(oj);
        while (lds.end[m] <= o) ++m;  // o < end[63]
        const uint64_t st = m ? lds.end[m - 1] : 0u;
        v[j] = stretch_word(lds, m, (o - st) >> 2);
      }
      if (full) {
        *reinterpret_cast<u32x4 *>(base + o0) = u32x4{v[0], v[1], v[2], v[3]};
      } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const int64_t oj = o0 + 4 * j;
          if (oj >= 0 && static_cast<uint64_t>(oj) < total) st32(base + oj, v[j]);
        }
      }
    }
  }
}

}  // namespace dev
}  // namespace xdrg
