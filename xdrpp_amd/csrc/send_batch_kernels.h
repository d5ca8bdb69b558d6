// The send batch (send_batch.hip): msg_sock::putmsg (xdrpp/msgsock.cc:121-134)
// for the messages of many streams and many connections at once.  The
// messages come as sources (a record-marked stream, its offsets and the
// connection of every entry, in any order) and leave as one stream in which
// every connection's messages are contiguous and in putmsg order, with one
// queue record per connection: wqueue_ / wsize_ of a fresh queue.  It is a
// stable sort by connection with a byte gather behind it:
//
//   k_sb_keys    one lane per entry g (source-major): its outcome, the item
//                (key << 32 | g) with key = the connection of a queued entry
//                and nconns, which sorts last, for every other; d_pos of the
//                others; per 256-entry tile the outcome counts and the
//                descents of the key sequence
//   k_tile_scan<1, 2, sb_key_totals>   d_counts from the tile sums, and
//                ctl->inorder = no descent: the order is the identity
//   k_sb_hist, k_sb_pass_scan, k_sb_scatter   one LSD radix pass over 8 bits
//                of the key, kSbSortTile items a workgroup: the (digit, tile)
//                counts digit-major, their exclusive scan (k_tile_scan's
//                rounds over 32-bit words), then every item to scan + its rank
//                in the tile among equal digits: ballots over the digit's bits within a
//                wave's 64 items, the wave's earlier rounds and the waves
//                before it through LDS.  No atomic decides a position.  All
//                three return at once when ctl->inorder is set.
//   k_sb_sizes   one lane per queue position j: conn_of, from, d_pos of its
//                entry, its bytes; tile sums
//   k_tile_scan<2, 2, gather_totals>
//   k_sb_emit    the stretch emit of batch_kernels.h without header words:
//                a wave's 64 queue positions are one contiguous stretch
//   k_sb_queues  one lane per connection: two binary searches of the sorted
//                keys give first and msgs, d_offsets gives begin and len
#pragma once
#include "batch_kernels.h"

namespace xdrg {
namespace dev {

constexpr uint32_t kSbItems = 8;                            // items a lane of a sort pass
constexpr uint32_t kSbSortTile = kTileThreads * kSbItems;   // XDRG_RPC_SEND_SORT_TILE
static_assert(kSbSortTile == XDRG_RPC_SEND_SORT_TILE, "the header names the sort tile");
static_assert(XDRG_RPC_MAX_SEND_SRCS == kMaxSrcs, "src_count_table serves the send sources");

// d_pos of an entry that is not queued
constexpr long long kSbPosDropped = -1, kSbPosEmpty = -2, kSbPosUnusable = -3;
enum : uint32_t { kSbQueued = 0, kSbDropped = 1, kSbEmpty = 2, kSbUnusable = 3, kSbAbsent = 4 };

struct sb_src {
  const uint8_t *bytes;
  const uint64_t *offsets;
  const uint32_t *conn;  // nullptr: every entry goes to conn_all
  const uint64_t *count;
  uint64_t bytes_len;
  uint32_t cap, conn_all;
};
struct sb_table {
  sb_src e[kMaxSrcs];
  uint32_t base[kMaxSrcs + 1];  // global number of each source's entry 0 (the caps before it)
};
static_assert(sizeof(sb_table) + 256 < 4096, "kernel arguments under 4 KiB");

struct sb_ctl {
  uint32_t inorder, rsv;
};

// Source and entry of global number g (g < base[nsrcs]): the last source
// whose base is at or below g (a source without entries shares its base with
// the next one).  A uniform loop: the bases are read with scalar loads.
__device__ __forceinline__ uint32_t sb_locate(const sb_table &T, uint32_t nsrcs, uint32_t g, uint32_t *k) {
  uint32_t s = 0;
  for (uint32_t i = 1; i < nsrcs; ++i) s = T.base[i] <= g ? i : s;
  *k = g - T.base[s];
  return s;
}

// The outcome of entry g and, when it is queued or dropped, its connection.
// Reads the entry's two offsets, its connection and, only for a span that is
// aligned, inside the stream and at least a mark long, the span's first word.
__device__ __forceinline__ uint32_t sb_outcome(const sb_table &T, uint32_t nsrcs, uint32_t g, uint64_t nconns,
                                               const uint32_t *__restrict__ closed, uint32_t *conn) {
  uint32_t k;
  const sb_src &S = T.e[sb_locate(T, nsrcs, g, &k)];
  *conn = 0;
  if (k >= src_count(S.count, S.cap)) return kSbAbsent;
  const uint64_t a = S.offsets[k], b = S.offsets[k + 1];
  if (a == b) return kSbEmpty;
  if (b < a || b > S.bytes_len || ((a | b) & 3u) || b - a < 4u || b - a - 4u > XDRG_MAX_MSG) return kSbUnusable;
  const uint32_t c = S.conn ? S.conn[k] : S.conn_all;
  if (c >= nconns) return kSbUnusable;
  if (ld32(S.bytes + a) != mark_word(static_cast<uint32_t>(b - a - 4u))) return kSbUnusable;
  *conn = c;
  return closed && closed[c] ? kSbDropped : kSbQueued;
}

__global__ __launch_bounds__(kTileThreads) void k_sb_keys(const sb_table T, uint32_t nsrcs, uint64_t entries,
                                                          uint64_t nconns, const uint32_t *__restrict__ closed,
                                                          unsigned long long *__restrict__ items,
                                                          long long *__restrict__ pos,
                                                          unsigned long long *__restrict__ tile_a,
                                                          unsigned long long *__restrict__ tile_b) {
  __shared__ uint32_t keys[kTileThreads];
  __shared__ unsigned long long wa[kTileThreads / 64], wb[kTileThreads / 64];
  const uint32_t tid = threadIdx.x;
  const uint64_t g = static_cast<uint64_t>(blockIdx.x) * kTileThreads + tid;
  const uint32_t sentinel = static_cast<uint32_t>(nconns);
  uint32_t key = sentinel, what = kSbAbsent, conn;
  if (g < entries) {
    what = sb_outcome(T, nsrcs, static_cast<uint32_t>(g), nconns, closed, &conn);
    if (what == kSbQueued) key = conn;
    items[g] = (static_cast<unsigned long long>(key) << 32) | g;
    if (pos && what != kSbQueued)
      pos[g] = what == kSbDropped ? kSbPosDropped : what == kSbUnusable ? kSbPosUnusable : kSbPosEmpty;
  }
  keys[tid] = key;
  // the key before this tile's first: one lane works it out again
  uint32_t before = 0;
  if (tid == 0 && g > 0 && g < entries)
    before = sb_outcome(T, nsrcs, static_cast<uint32_t>(g - 1), nconns, closed, &conn) == kSbQueued ? conn : sentinel;
  __syncthreads();
  const uint32_t prev = tid ? keys[tid - 1] : before;
  const bool descent = g < entries && prev > key;
  // queued | dropped << 32 and empty | descents << 32: no field reaches 2^32
  unsigned long long va = what == kSbQueued ? 1ull : what == kSbDropped ? 1ull << 32 : 0ull;
  unsigned long long vb = (what == kSbEmpty ? 1ull : 0ull) | (descent ? 1ull << 32 : 0ull);
  for (int o = 32; o > 0; o >>= 1) {
    va += __shfl_xor(va, o, 64);
    vb += __shfl_xor(vb, o, 64);
  }
  if ((tid & 63u) == 0u) {
    wa[tid >> 6] = va;
    wb[tid >> 6] = vb;
  }
  __syncthreads();
  if (tid == 0) {
    unsigned long long sa = 0, sb = 0;
    for (uint32_t k = 0; k < kTileThreads / 64; ++k) {
      sa += wa[k];
      sb += wb[k];
    }
    tile_a[blockIdx.x] = sa;
    tile_b[blockIdx.x] = sb;
  }
}

// counts (may be nullptr) = {queued, dropped, empty, unusable}: the unusable
// are the used entries of every source less the rest.
struct sb_key_totals {
  src_count_table N;
  uint32_t nsrcs;
  uint64_t *counts;
  sb_ctl *ctl;
  __device__ void operator()(const unsigned long long (&t)[2], uint32_t lane) const {
    const unsigned long long used = counts ? src_entries(N, nsrcs, lane) : 0ull;
    if (lane) return;
    const unsigned long long queued = t[0] & 0xffffffffull, dropped = t[0] >> 32, empty = t[1] & 0xffffffffull;
    ctl->inorder = (t[1] >> 32) == 0ull;
    if (counts) {
      counts[0] = queued;
      counts[1] = dropped;
      counts[2] = empty;
      counts[3] = used - queued - dropped - empty;
    }
  }
};

// ------------------------------------------------------------ a radix pass
// Item i of round r of wave w of tile t is t * kSbSortTile + w * 64 * kSbItems
// + r * 64 + lane: a wave's rounds, and a tile's waves, follow each other in
// item order.
__device__ __forceinline__ uint64_t sb_item(uint32_t round) {
  return static_cast<uint64_t>(blockIdx.x) * kSbSortTile + (threadIdx.x >> 6) * (64u * kSbItems) + round * 64u +
         (threadIdx.x & 63u);
}
__device__ __forceinline__ uint32_t sb_digit(unsigned long long item, uint32_t shift) {
  return static_cast<uint32_t>(item >> (32u + shift)) & 255u;
}

// counts[d * nt + t] = the items of tile t with digit d.  Sums: the order of
// the LDS adds does not show.
__global__ __launch_bounds__(kTileThreads) void k_sb_hist(const sb_ctl *__restrict__ ctl,
                                                          const unsigned long long *__restrict__ in, uint64_t n,
                                                          uint32_t shift, uint64_t nt,
                                                          uint32_t *__restrict__ counts) {
  if (ctl->inorder) return;
  __shared__ uint32_t hist[256];
  static_assert(kTileThreads == 256, "one lane per digit");
  hist[threadIdx.x] = 0u;
  __syncthreads();
#pragma unroll
  for (uint32_t r = 0; r < kSbItems; ++r) {
    const uint64_t i = sb_item(r);
    if (i < n) atomicAdd(&hist[sb_digit(in[i], shift)], 1u);
  }
  __syncthreads();
  counts[static_cast<uint64_t>(threadIdx.x) * nt + blockIdx.x] = hist[threadIdx.x];
}

// The exclusive scan of the nb = 256 nt counts, in place: k_tile_scan's rounds
// over 32-bit words (no offset reaches 2^32), in a kernel of its own because
// it has to stand aside with the rest of the pass.  A lane takes 16
// consecutive words a round as four 16-byte loads (nb is a multiple of 256;
// the workspace need only be 8-aligned, hence ld16u), so 1M entries are 8
// rounds, not 128 (29 us a pass against 70 at four words a lane).
constexpr uint32_t kSbScanWords = 16;
__global__ __launch_bounds__(kScanThreads) void k_sb_pass_scan(const sb_ctl *__restrict__ ctl,
                                                               uint32_t *__restrict__ counts, uint64_t nb) {
  if (ctl->inorder) return;
  __shared__ uint32_t ws[kScanThreads / 64];
  const uint32_t tid = threadIdx.x, lane = tid & 63u, wid = tid >> 6;
  uint32_t carry = 0;
  for (uint64_t t0 = 0; t0 < nb; t0 += kSbScanWords * kScanThreads) {
    const uint64_t j = t0 + kSbScanWords * tid;
    u32x4 v[kSbScanWords / 4];
    uint32_t sum = 0;
#pragma unroll
    for (uint32_t q = 0; q < kSbScanWords / 4; ++q) {
      v[q] = j + 4u * q < nb ? ld16u(reinterpret_cast<const uint8_t *>(counts + j + 4u * q)) : u32x4{0u, 0u, 0u, 0u};
      sum += v[q].x + v[q].y + v[q].z + v[q].w;
    }
    const uint32_t iv = wave_incl_scan(sum);
    if (lane == 63u) ws[wid] = iv;
    __syncthreads();
    uint32_t at = carry, total = 0;
    for (uint32_t k = 0; k < kScanThreads / 64; ++k) {
      if (k < wid) at += ws[k];
      total += ws[k];
    }
    at += iv - sum;
#pragma unroll
    for (uint32_t q = 0; q < kSbScanWords / 4; ++q) {
      const u32x4 o{at, at + v[q].x, at + v[q].x + v[q].y, at + v[q].x + v[q].y + v[q].z};
      at = o.w + v[q].w;
      if (j + 4u * q < nb) st16u(reinterpret_cast<uint8_t *>(counts + j + 4u * q), o);
    }
    carry += total;
    __syncthreads();  // ws reused by the next round
  }
}

// The lanes of the wave that are `valid` and hold digit d.
__device__ __forceinline__ unsigned long long sb_match(uint32_t d, bool valid) {
  unsigned long long m = __ballot(valid);
#pragma unroll
  for (uint32_t b = 0; b < 8; ++b) {
    const bool bit = (d >> b) & 1u;
    const unsigned long long has = __ballot(bit);
    m &= bit ? has : ~has;
  }
  return m;
}

__global__ __launch_bounds__(kTileThreads) void k_sb_scatter(const sb_ctl *__restrict__ ctl,
                                                             const unsigned long long *__restrict__ in, uint64_t n,
                                                             uint32_t shift, uint64_t nt,
                                                             const uint32_t *__restrict__ base,
                                                             unsigned long long *__restrict__ out) {
  if (ctl->inorder) return;
  __shared__ uint32_t wcnt[kTileThreads / 64][256];  // a wave's items so far, by digit
  const uint32_t tid = threadIdx.x, lane = tid & 63u, wid = tid >> 6;
  for (uint32_t k = 0; k < kTileThreads / 64; ++k) wcnt[k][tid] = 0u;
  __syncthreads();
  unsigned long long v[kSbItems];
  uint32_t rank[kSbItems];
#pragma unroll
  for (uint32_t r = 0; r < kSbItems; ++r) {
    const bool valid = sb_item(r) < n;
    v[r] = valid ? in[sb_item(r)] : 0ull;
    const uint32_t d = sb_digit(v[r], shift);
    const unsigned long long m = sb_match(d, valid);
    const uint32_t below = __popcll(m & ((1ull << lane) - 1ull));
    const uint32_t prior = wcnt[wid][d];
    wave_sync();  // every lane has read the count before the first of its digit moves it on
    if (valid && below == 0u) wcnt[wid][d] = prior + static_cast<uint32_t>(__popcll(m));
    wave_sync();
    rank[r] = prior + below;
  }
  __syncthreads();
#pragma unroll
  for (uint32_t r = 0; r < kSbItems; ++r) {
    if (sb_item(r) >= n) continue;
    const uint32_t d = sb_digit(v[r], shift);
    uint64_t at = base[static_cast<uint64_t>(d) * nt + blockIdx.x] + rank[r];
    for (uint32_t k = 0; k < wid; ++k) at += wcnt[k][d];
    if (at < n) out[at] = v[r];
  }
}

// ------------------------------------------------- count -> scan -> emit
// The sorted items: where the passes left them, or where k_sb_keys wrote them
// when the passes stood aside.
struct sb_sorted {
  const sb_ctl *ctl;
  const unsigned long long *keyed, *passed;
  __device__ __forceinline__ const unsigned long long *get() const { return ctl->inorder ? keyed : passed; }
};

// Queue position j: whether a message stands there, its entry's span.
__device__ __forceinline__ bool sb_queued_at(const unsigned long long *__restrict__ sorted, uint64_t j, uint64_t entries,
                                             uint64_t nconns, const sb_table &T, uint32_t nsrcs, uint32_t *key,
                                             uint32_t *g, uint32_t *s, uint32_t *k, uint64_t *a, uint64_t *b) {
  if (j >= entries) return false;
  const unsigned long long it = sorted[j];
  *key = static_cast<uint32_t>(it >> 32);
  *g = static_cast<uint32_t>(it);
  if (*key >= nconns || *g >= entries) return false;
  *s = sb_locate(T, nsrcs, *g, k);
  *a = T.e[*s].offsets[*k];
  *b = T.e[*s].offsets[*k + 1];
  return true;
}

__global__ __launch_bounds__(kTileThreads) void k_sb_sizes(const sb_sorted sorted, uint64_t entries, uint64_t nconns,
                                                           const sb_table T, uint32_t nsrcs,
                                                           uint32_t *__restrict__ conn_of,
                                                           uint64_t *__restrict__ from, long long *__restrict__ pos,
                                                           unsigned long long *__restrict__ tile_cnt,
                                                           unsigned long long *__restrict__ tile_bytes) {
  const uint64_t j = static_cast<uint64_t>(blockIdx.x) * kTileThreads + threadIdx.x;
  uint32_t key, g, s, k;
  uint64_t a = 0, b = 0;
  const bool present = sb_queued_at(sorted.get(), j, entries, nconns, T, nsrcs, &key, &g, &s, &k, &a, &b);
  if (present) {
    conn_of[j] = key;
    from[j] = (static_cast<uint64_t>(s) << 32) | k;
    if (pos) pos[g] = static_cast<long long>(j);
  }
  tile_reduce(present ? b - a : 0ull, present, tile_bytes, tile_cnt);
}

// A wave's stretch without header words: every word of a message comes from
// its source.
template <>
struct wave_stretch<0, false, 0> {
  static constexpr uint32_t kPayloadAt = 0;
  unsigned long long end[64];
  const uint8_t *src[64];
  uint32_t w[1][1];  // never read: words() is 0
  __device__ __forceinline__ uint32_t words(uint32_t) const { return 0; }
};
using sb_wave_lds = wave_stretch<0, false, 0>;

template <int W>
__global__ __launch_bounds__(kTileThreads) void k_sb_emit(const sb_sorted sorted, uint64_t entries, uint64_t nconns,
                                                          const sb_table T, uint32_t nsrcs, uint8_t *__restrict__ out,
                                                          uint64_t cap, uint64_t *__restrict__ offsets,
                                                          const unsigned long long *__restrict__ tile_bytes,
                                                          unsigned long long *err) {
  __shared__ sb_wave_lds lds[kTileThreads / 64];
  const uint32_t lane = threadIdx.x & 63u;
  const uint64_t j = static_cast<uint64_t>(blockIdx.x) * kTileThreads + threadIdx.x;
  sb_wave_lds &L = lds[threadIdx.x >> 6];
  uint32_t key, g, s = 0, k;
  uint64_t a = 0, b = 0;
  const bool present = sb_queued_at(sorted.get(), j, entries, nconns, T, nsrcs, &key, &g, &s, &k, &a, &b);
  const stretch_at p = stretch_place(present ? b - a : 0ull, present, j, tile_bytes, cap, err, L.end, [&](uint64_t at) {
    if (present) offsets[j] = at;
  });
  L.src[lane] = present ? T.e[s].bytes + a : nullptr;
  __syncthreads();
  stretch_write<W>(L, out + p.wbase, lane);
}

// One lane per connection.  The first position whose key is at or above c.
__device__ __forceinline__ uint64_t sb_lower(const unsigned long long *__restrict__ sorted, uint64_t n, uint64_t c) {
  uint64_t lo = 0, hi = n;
  while (lo < hi) {
    const uint64_t mid = lo + ((hi - lo) >> 1);
    if ((sorted[mid] >> 32) < c) lo = mid + 1; else hi = mid;
  }
  return lo;
}

// offsets[0 .. m] are written by then (k_sb_emit, gather_totals), and every
// position found here is at or below m: the keys from m on are nconns.
__global__ __launch_bounds__(kTileThreads) void k_sb_queues(const sb_sorted sorted, uint64_t entries, uint64_t nconns,
                                                            const uint64_t *__restrict__ offsets,
                                                            xdrg_rpc_wqueue *__restrict__ queues) {
  const uint64_t c = static_cast<uint64_t>(blockIdx.x) * kTileThreads + threadIdx.x;
  if (c >= nconns) return;
  const unsigned long long *items = sorted.get();
  const uint64_t lo = sb_lower(items, entries, c), hi = sb_lower(items, entries, c + 1);
  const uint64_t begin = offsets[lo], end = offsets[hi];
  queues[c] = xdrg_rpc_wqueue{lo, hi - lo, begin, end - begin};
}

}  // namespace dev
}  // namespace xdrg
