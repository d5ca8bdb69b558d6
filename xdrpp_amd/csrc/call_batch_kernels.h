// The asynchronous client's send half for a whole batch (call_batch.hip):
// asynchronous_client_base::invoke (xdrpp/arpc.h:41-59) takes an xid from
// rpc_sock::get_xid (msgsock.h:118-122), marshals xdr_to_msg(hdr, args...)
// and rpc_sock::send_call (msgsock.cc:227-232) remembers the call.  Here the
// arguments come as sources (what xdrg_encode wrote for one procedure, and
// the call position of each of them) and the batch's calls leave as one
// record-marked stream in call order.
//
//   k_cb_next_xids    one lane per xid: the (k+1)-th value after last_xid that
//                     is not pending, by two binary searches of the table
//   k_cb_fill         owner[i] = all ones (no entry)
//   k_cb_claim        one lane per source entry, every source in one launch:
//                     a usable entry claims its position with a 64-bit
//                     atomicMin of (source << 32 | position), so the lowest
//                     entry wins whatever the order the lanes run in
//   k_cb_sizes        one lane per position: its message bytes (44 + L with a
//                     winning entry, else 0) and whether an entry won it, both
//                     summed per 256-position tile
//   k_cb_scan         exclusive scan of the tile bytes in one workgroup; the
//                     total; counts[0] = n - the winners, counts[1] = the
//                     sources' entries - the winners (tile sums, no atomic on
//                     one word: DESIGN.md 7.2.3)
//   k_cb_emit         offsets and d_sent a lane per position; the bytes a wave
//                     per run of 64 positions: their messages are one
//                     contiguous stretch of the output, written with
//                     consecutive lanes on consecutive aligned 16-byte chunks,
//                     each chunk's message found by a binary search of the
//                     wave's 64 byte ends in LDS.  The mark and the ten header
//                     words come from LDS, the argument bytes from the winning
//                     source.
//   k_cb_pending_add  one lane per old and per new entry of the pending table:
//                     its place in the merged table by binary searches
//
// Everything is whole aligned words by contract (unusable entries never
// claim), so there is no byte path.
#pragma once
#include <hip/hip_runtime.h>

#include "dev_common.h"

namespace xdrg {
namespace dev {

constexpr uint32_t kCbThreads = 256;
constexpr unsigned long long kCbNoOwner = ~0ull;
constexpr uint32_t kCbHdrWords = 11;  // mark + the call header (arpc.h:44-48: xid, CALL, 2, prog, vers, proc, cred, verf)

// What the claim needs of a source.  A source without arguments (d_bytes
// NULL) arrives with offsets = nullptr and fixed = 0: every span is [0, 0).
struct cb_claim_src {
  const uint64_t *index;
  const uint64_t *count;    // nullptr: cap entries
  const uint64_t *offsets;  // nullptr: fixed-size arguments
  uint64_t bytes_len;
  uint32_t cap, fixed;
};
struct cb_claim_table {
  cb_claim_src e[XDRG_RPC_MAX_ARG_SRCS];
  uint32_t blk[XDRG_RPC_MAX_ARG_SRCS + 1];  // first workgroup of each source
};

// What the sizes need of a source: how long a winning entry is.
struct cb_size_src {
  const uint64_t *offsets;
  uint64_t fixed;
};
struct cb_size_table {
  cb_size_src e[XDRG_RPC_MAX_ARG_SRCS];
};

// What the emit needs: where a winning entry's bytes are, and the words its
// procedure puts into the header and the pending table.
struct cb_emit_src {
  const uint8_t *bytes;
  const uint64_t *offsets;
  uint32_t fixed, res;
  uint32_t prog, vers, proc, rsv;
};
struct cb_emit_table {
  cb_emit_src e[XDRG_RPC_MAX_ARG_SRCS];
};

// The counts alone, for the kernel that sums the entries.
struct cb_count_table {
  const uint64_t *count[XDRG_RPC_MAX_ARG_SRCS];
  uint32_t cap[XDRG_RPC_MAX_ARG_SRCS];
};

__device__ __forceinline__ uint64_t cb_count(const uint64_t *count, uint32_t cap) {
  const uint64_t c = count ? *count : cap;
  return c < cap ? c : cap;
}

// The entries of every source (lanes 0..63 of the calling wave, all active).
__device__ __forceinline__ unsigned long long cb_entries(const cb_count_table &T, uint32_t nsrcs, uint32_t lane) {
  unsigned long long c = 0;
  for (uint32_t k = 0; k < nsrcs; ++k)  // uniform k: the table is read with scalar loads
    if (lane == k) c = cb_count(T.count[k], T.cap[k]);
  for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o, 64);
  return c;
}

__device__ __forceinline__ uint64_t cb_incl_scan64(uint64_t x) {
  const uint32_t lane = __lane_id();
  for (int o = 1; o < 64; o <<= 1) {
    const uint64_t y = __shfl_up(x, o, 64);
    if (lane >= static_cast<uint32_t>(o)) x += y;
  }
  return x;
}

// ------------------------------------------------------------- next xids
// The entries of the sorted table whose xid is below x.
__device__ __forceinline__ uint64_t cb_lower_bound(const xdrg_rpc_call *__restrict__ calls, uint64_t ncalls,
                                                   uint32_t x) {
  uint64_t lo = 0, hi = ncalls;
  while (lo < hi) {
    const uint64_t mid = lo + ((hi - lo) >> 1);
    if (calls[mid].xid < x) lo = mid + 1; else hi = mid;
  }
  return lo;
}

// rpc_sock::get_xid() n times, each followed by send_call (msgsock.h:118-122).
// In rotated coordinates r(x) = (x - last - 1) mod 2^32 the table, read from
// its split point s = lower_bound(last + 1) on and around its end, is
// ascending: R[0] < R[1] < ...  The k-th free value is k + j for the smallest
// j with R[j] - j > k (j pending values lie at or below it); j = ncalls when
// there is none.  ncalls + n <= 2^32 - 1, so the value exists.
__global__ __launch_bounds__(kCbThreads) void k_cb_next_xids(const xdrg_rpc_call *__restrict__ calls,
                                                             uint64_t ncalls, uint32_t last, uint64_t n,
                                                             uint32_t *__restrict__ xids) {
  const uint64_t k = static_cast<uint64_t>(blockIdx.x) * kCbThreads + threadIdx.x;
  if (k >= n) return;
  const uint32_t base = last + 1u;
  const uint64_t s = cb_lower_bound(calls, ncalls, base);
  uint64_t lo = 0, hi = ncalls;
  while (lo < hi) {
    const uint64_t mid = lo + ((hi - lo) >> 1);
    const uint64_t at = s + mid < ncalls ? s + mid : s + mid - ncalls;
    const uint64_t r = static_cast<uint32_t>(calls[at].xid - base);
    // r >= mid in a table that keeps the contract; a signed compare keeps a
    // broken one from wrapping
    if (static_cast<int64_t>(r) - static_cast<int64_t>(mid) > static_cast<int64_t>(k)) hi = mid; else lo = mid + 1;
  }
  xids[k] = base + static_cast<uint32_t>(k) + static_cast<uint32_t>(lo);
}

// ----------------------------------------------------------- pending add
// The first entry of d_new past the wrap: the smallest k with xid_k < xid_0
// (n when the xids did not wrap).
__device__ __forceinline__ uint64_t cb_wrap_point(const xdrg_rpc_call *__restrict__ fresh, uint64_t n) {
  const uint32_t x0 = fresh[0].xid;
  uint64_t lo = 0, hi = n;
  while (lo < hi) {
    const uint64_t mid = lo + ((hi - lo) >> 1);
    if (fresh[mid].xid >= x0) lo = mid + 1; else hi = mid;
  }
  return lo;
}

// calls_ after the sends: lanes 0..ncalls-1 place the old entries, the next n
// the new ones.  Every position written is below ncalls + n whatever the
// arrays hold (a lower bound is at most its array's length).
__global__ __launch_bounds__(kCbThreads) void k_cb_pending_add(const xdrg_rpc_call *__restrict__ calls,
                                                               uint64_t ncalls,
                                                               const xdrg_rpc_call *__restrict__ fresh, uint64_t n,
                                                               xdrg_rpc_call *__restrict__ merged,
                                                               uint64_t *__restrict__ old_pos,
                                                               uint64_t *__restrict__ new_pos) {
  const uint64_t t = static_cast<uint64_t>(blockIdx.x) * kCbThreads + threadIdx.x;
  if (t >= ncalls + n) return;
  const uint64_t w = n ? cb_wrap_point(fresh, n) : 0u;
  if (t < ncalls) {
    const xdrg_rpc_call c = calls[t];
    // the new entries below it: in the run before the wrap and in the one after
    const uint64_t below = cb_lower_bound(fresh, w, c.xid) + cb_lower_bound(fresh + w, n - w, c.xid);
    merged[t + below] = c;
    if (old_pos) old_pos[t] = t + below;
  } else {
    const uint64_t k = t - ncalls;
    const xdrg_rpc_call c = fresh[k];
    const uint64_t rank = k < w ? (n - w) + k : k - w;
    const uint64_t at = cb_lower_bound(calls, ncalls, c.xid) + rank;
    merged[at] = c;
    if (new_pos) new_pos[k] = at;
  }
}

// ------------------------------------------------------------ call stream
__global__ __launch_bounds__(kCbThreads) void k_cb_fill(unsigned long long *__restrict__ owner, uint64_t n) {
  const uint64_t i = static_cast<uint64_t>(blockIdx.x) * kCbThreads + threadIdx.x;
  if (i < n) owner[i] = kCbNoOwner;
}

// n == 0: no position, every entry is unused.
__global__ __launch_bounds__(64) void k_cb_count_entries(const cb_count_table T, uint32_t nsrcs,
                                                         unsigned long long *__restrict__ counts) {
  const unsigned long long c = cb_entries(T, nsrcs, threadIdx.x);
  if (threadIdx.x == 0) { counts[0] = 0; counts[1] = c; }
}

// One lane per entry.  The workgroup's source is found by a uniform loop over
// the table (kernel arguments: scalar loads).
__global__ __launch_bounds__(kCbThreads) void k_cb_claim(uint64_t n, const cb_claim_table T, uint32_t nsrcs,
                                                         unsigned long long *__restrict__ owner) {
  uint32_t s = 0;
  for (uint32_t k = 1; k < nsrcs; ++k) s = T.blk[k] <= blockIdx.x ? k : s;
  const cb_claim_src S = T.e[s];
  const uint64_t pos = static_cast<uint64_t>(blockIdx.x - T.blk[s]) * kCbThreads + threadIdx.x;
  if (pos >= cb_count(S.count, S.cap)) return;
  const uint64_t i = S.index[pos];
  if (i < n) {
    const uint64_t a = S.offsets ? S.offsets[pos] : pos * S.fixed;
    const uint64_t b = S.offsets ? S.offsets[pos + 1] : a + S.fixed;
    if (b >= a && b <= S.bytes_len && !((a | b) & 3u) && b - a <= XDRG_MAX_MSG - 40u)
      atomicMin(owner + i, (static_cast<unsigned long long>(s) << 32) | pos);
  }
}

__device__ __forceinline__ uint32_t cb_src_of(unsigned long long own) {
  return static_cast<uint32_t>(own >> 32) & (XDRG_RPC_MAX_ARG_SRCS - 1u);
}

__global__ __launch_bounds__(kCbThreads) void k_cb_sizes(uint64_t n, const unsigned long long *__restrict__ owner,
                                                         const cb_size_table T,
                                                         unsigned long long *__restrict__ tile_bytes,
                                                         unsigned long long *__restrict__ tile_won) {
  __shared__ unsigned long long wb[kCbThreads / 64];
  __shared__ uint32_t ww[kCbThreads / 64];
  const uint64_t i = static_cast<uint64_t>(blockIdx.x) * kCbThreads + threadIdx.x;
  unsigned long long t = 0;
  bool won = false;
  if (i < n) {
    const unsigned long long own = owner[i];
    won = own != kCbNoOwner;
    if (won) {
      const cb_size_src S = T.e[cb_src_of(own)];
      const uint64_t pos = own & 0xffffffffull;
      const uint64_t a = S.offsets ? S.offsets[pos] : pos * S.fixed;
      const uint64_t b = S.offsets ? S.offsets[pos + 1] : a + S.fixed;
      t = 4u * kCbHdrWords + (b - a);  // the claim has checked the span
    }
  }
  const unsigned long long m = __ballot(won);
  for (int o = 32; o > 0; o >>= 1) t += __shfl_xor(t, o, 64);
  if ((threadIdx.x & 63u) == 0u) {
    wb[threadIdx.x >> 6] = t;
    ww[threadIdx.x >> 6] = __popcll(m);
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    unsigned long long sb = 0, sw = 0;
    for (uint32_t k = 0; k < kCbThreads / 64; ++k) { sb += wb[k]; sw += ww[k]; }
    tile_bytes[blockIdx.x] = sb;
    tile_won[blockIdx.x] = sw;
  }
}

// Exclusive scan in place of the nb tile bytes; the total to offsets[n] and
// status->total_bytes; counts[0] = the positions no entry won, counts[1] =
// the entries of every source less the winners.  One workgroup of 1024.
__global__ __launch_bounds__(1024) void k_cb_scan(unsigned long long *__restrict__ tile_bytes,
                                                  const unsigned long long *__restrict__ tile_won, uint64_t nb,
                                                  uint64_t n, const cb_count_table T, uint32_t nsrcs,
                                                  uint64_t *__restrict__ total_at, xdrg_status *status,
                                                  unsigned long long *__restrict__ counts) {
  __shared__ unsigned long long wb[16], ww[16];
  const uint32_t tid = threadIdx.x, lane = tid & 63u, wid = tid >> 6;
  unsigned long long carry = 0, won = 0;
  for (uint64_t t0 = 0; t0 < nb; t0 += 1024u) {
    const uint64_t j = t0 + tid;
    const unsigned long long b = j < nb ? tile_bytes[j] : 0ull;
    unsigned long long w = j < nb ? tile_won[j] : 0ull;
    const unsigned long long ib = cb_incl_scan64(b);
    for (int o = 32; o > 0; o >>= 1) w += __shfl_xor(w, o, 64);
    if (lane == 63u) { wb[wid] = ib; ww[wid] = w; }
    __syncthreads();
    unsigned long long bb = carry, tb = 0;
    for (uint32_t k = 0; k < 16; ++k) {
      if (k < wid) bb += wb[k];
      tb += wb[k];
      won += ww[k];
    }
    if (j < nb) tile_bytes[j] = bb + ib - b;
    carry += tb;
    __syncthreads();  // wb / ww reused by the next round
  }
  if (wid == 0) {
    const unsigned long long entries = counts ? cb_entries(T, nsrcs, lane) : 0ull;
    if (lane == 0) {
      *total_at = carry;
      status->total_bytes = carry;
      if (counts) { counts[0] = n - won; counts[1] = entries - won; }
    }
  }
}

// The wave's LDS: byte ends and argument pointers of its 64 positions and the
// eleven words each message starts with (one column per position: a lane
// writes its column without bank conflicts).
struct cb_wave_lds {
  unsigned long long end[64];
  const uint8_t *src[64];
  uint32_t w[kCbHdrWords][64];
};

// Word `k` of message `m` of the wave.
__device__ __forceinline__ uint32_t cb_word(const cb_wave_lds &L, uint32_t m, uint64_t k) {
  return k < kCbHdrWords ? L.w[k][m] : ld32(L.src[m] + 4u * (k - kCbHdrWords));
}

// The first position of the wave whose end is past `off` (off < end[63]).
__device__ __forceinline__ uint32_t cb_find(const cb_wave_lds &L, uint64_t off) {
  uint32_t lo = 0, hi = 63;
  while (lo < hi) {
    const uint32_t mid = (lo + hi) >> 1;
    if (L.end[mid] > off) hi = mid; else lo = mid + 1;
  }
  return lo;
}

__global__ __launch_bounds__(kCbThreads) void k_cb_emit(const uint32_t *__restrict__ xids, uint64_t n,
                                                        const unsigned long long *__restrict__ owner,
                                                        const cb_emit_table T, uint8_t *__restrict__ out,
                                                        uint64_t cap, uint64_t *__restrict__ offsets,
                                                        xdrg_rpc_call *__restrict__ sent,
                                                        const unsigned long long *__restrict__ tile_bytes,
                                                        unsigned long long *err) {
  __shared__ unsigned long long wb[kCbThreads / 64];
  __shared__ cb_wave_lds lds[kCbThreads / 64];
  const uint32_t tid = threadIdx.x, lane = tid & 63u, wid = tid >> 6;
  const uint64_t i = static_cast<uint64_t>(blockIdx.x) * kCbThreads + tid;
  cb_wave_lds &L = lds[wid];
  uint32_t bytes = 0;
  const uint8_t *src = nullptr;
  if (i < n) {
    const uint32_t xid = xids[i];
    const unsigned long long own = owner[i];
    uint32_t res = XDRG_RPC_RES_UNSENT;
    if (own != kCbNoOwner) {
      const cb_emit_src S = T.e[cb_src_of(own)];
      const uint64_t pos = own & 0xffffffffull;
      const uint64_t a = S.offsets ? S.offsets[pos] : pos * S.fixed;
      const uint64_t b = S.offsets ? S.offsets[pos + 1] : a + S.fixed;
      src = S.bytes + a;
      bytes = 4u * kCbHdrWords + static_cast<uint32_t>(b - a);
      res = S.res;
      // message_t::alloc mark (marshal.cc:15-31), then rpc_msg's words (arpc.h:44-48)
      L.w[0][lane] = mark_word(bytes - 4u);
      L.w[1][lane] = bswap32(xid);
      L.w[2][lane] = 0u;  // CALL
      L.w[3][lane] = bswap32(2u);
      L.w[4][lane] = bswap32(S.prog);
      L.w[5][lane] = bswap32(S.vers);
      L.w[6][lane] = bswap32(S.proc);
      L.w[7][lane] = 0u;  // cred: AUTH_NONE, body<>
      L.w[8][lane] = 0u;
      L.w[9][lane] = 0u;  // verf
      L.w[10][lane] = 0u;
    }
    if (sent) sent[i] = xdrg_rpc_call{xid, res};
  }
  const uint64_t ib = cb_incl_scan64(bytes);
  if (lane == 63u) wb[wid] = ib;
  __syncthreads();
  uint64_t wbase = tile_bytes[blockIdx.x];  // where the wave's stretch starts
  for (uint32_t k = 0; k < wid; ++k) wbase += wb[k];
  const uint64_t at = wbase + ib - bytes;
  if (i < n) offsets[i] = at;
  bool fits = false;
  if (bytes) {
    fits = at <= cap && bytes <= cap - at;
    if (!fits) {  // xdr_generic_put::check (marshal.h:104-108)
      const unsigned long long key = (static_cast<unsigned long long>(i) << 24) |
                                     (static_cast<unsigned long long>(kOpRecordLevel) << 8) | XDRG_ERR_OVERFLOW_PUT;
      atomicMin(err, key);
    }
  }
  // the messages that fit are a prefix of the wave's stretch
  L.end[lane] = cb_incl_scan64(fits ? bytes : 0u);
  L.src[lane] = src;
  __syncthreads();
  const uint64_t total = L.end[63];
  uint8_t *base = out + wbase;
  // Aligned 16-byte chunks of the output: chunk c holds the stretch's bytes
  // [16 c - pre, 16 c - pre + 16), the first and the last may be partial.
  const uint64_t pre = reinterpret_cast<uintptr_t>(base) & 15u;
  const uint64_t nchunks = total ? (pre + total + 15u) >> 4 : 0u;
  for (uint64_t c = lane; c < nchunks; c += 64u) {
    const int64_t o0 = static_cast<int64_t>(16u * c) - static_cast<int64_t>(pre);
    const bool full = o0 >= 0 && static_cast<uint64_t>(o0) + 16u <= total;
    const uint64_t first = o0 < 0 ? 0u : static_cast<uint64_t>(o0);
    uint32_t m = cb_find(L, first);
    const uint64_t start = m ? L.end[m - 1] : 0u, k0 = (first - start) >> 2;
    if (full && k0 >= kCbHdrWords && first + 16u <= L.end[m]) {  // four words of one argument run
      *reinterpret_cast<u32x4 *>(base + o0) = ld16u(L.src[m] + 4u * (k0 - kCbHdrWords));
      continue;
    }
    uint32_t v[4] = {0u, 0u, 0u, 0u};
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int64_t oj = o0 + 4 * j;
      if (oj < 0 || static_cast<uint64_t>(oj) >= total) continue;
      const uint64_t o = static_cast<uint64_t>(oj);
      while (L.end[m] <= o) ++m;  // o < end[63]
      const uint64_t st = m ? L.end[m - 1] : 0u;
      v[j] = cb_word(L, m, (o - st) >> 2);
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

}  // namespace dev
}  // namespace xdrg
