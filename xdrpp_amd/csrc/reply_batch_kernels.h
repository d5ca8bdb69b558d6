// The server's reply step for a whole dispatched batch (reply_batch.hip):
// srpc_server::run (xdrpp/srpc.cc:83-88) writes one reply per answered call in
// call order -- xdr_to_msg(rpc_success_hdr(xid), *res) (srpc.h:152,
// server.h:27-49) for a call its handler served, one of the rpc_*_msg error
// replies (server.cc:8-67) for a call that failed.  Here the results come as
// sources (what xdrg_encode wrote, and the message each result answers) and
// the batch's replies leave as one record-marked stream in message order.
//
//   k_rb_fill    owner[i] = all ones (no entry)
//   k_rb_claim   one lane per source entry, every source in one launch: a
//                usable entry claims its message with a 64-bit atomicMin of
//                (source << 32 | position), so the lowest entry wins whatever
//                the order the lanes run in
//   k_rb_sizes   one lane per message: its reply bytes (error reply by action,
//                28 + L for a DISPATCH with a winning entry, else 0) and
//                whether an entry won it, both summed per 256-message tile
//   k_rb_scan    exclusive scan of the tile bytes in one workgroup; the total;
//                *unused = the sources' entries - the winners (no atomic on
//                one word: 16K waves adding to *unused cost more than the
//                copy)
//   k_rb_emit    offsets a lane per message; the bytes a wave per run of 64
//                messages: their replies are one contiguous stretch of the
//                output, written with consecutive lanes on consecutive words
//                (W = 4) or on consecutive aligned 16-byte chunks (W = 16),
//                each word's message found by a binary search of the wave's
//                64 byte ends in LDS.  The words of an error reply and words
//                0..6 of a success reply come from LDS, the result bytes from
//                the winning source.
//
// Everything is whole aligned words by contract (unusable entries never
// claim), so there is no byte path.
#pragma once
#include <hip/hip_runtime.h>

#include "dev_common.h"

namespace xdrg {
namespace dev {

constexpr uint32_t kRbThreads = 256;
constexpr unsigned long long kRbNoOwner = ~0ull;
constexpr uint32_t kRbHdrWords = 7;  // mark + rpc_success_hdr (server.h:27-49)
constexpr uint32_t kRbMaxWords = 9;  // the longest error reply (PROG_MISMATCH)

// What the claim needs of a source.  A void source (d_bytes NULL) arrives
// with offsets = nullptr and fixed = 0: every span is [0, 0).
struct rb_claim_src {
  const uint64_t *index;
  const uint64_t *count;    // nullptr: cap entries
  const uint64_t *offsets;  // nullptr: fixed-size results
  uint64_t bytes_len;
  uint32_t cap, fixed;
};
struct rb_claim_table {
  rb_claim_src e[XDRG_RPC_MAX_RESULT_SRCS];
  uint32_t blk[XDRG_RPC_MAX_RESULT_SRCS + 1];  // first workgroup of each source
};

// What the sizes and the emit need of a source: where a winning entry's bytes
// are.
struct rb_span_src {
  const uint8_t *bytes;
  const uint64_t *offsets;
  uint64_t fixed;
};
struct rb_span_table {
  rb_span_src e[XDRG_RPC_MAX_RESULT_SRCS];
};

// The counts alone, for the kernel that sums the entries.
struct rb_count_table {
  const uint64_t *count[XDRG_RPC_MAX_RESULT_SRCS];
  uint32_t cap[XDRG_RPC_MAX_RESULT_SRCS];
};

__device__ __forceinline__ uint64_t rb_count(const uint64_t *count, uint32_t cap) {
  const uint64_t c = count ? *count : cap;
  return c < cap ? c : cap;
}

// The entries of every source (lanes 0..63 of the calling wave, all active).
__device__ __forceinline__ unsigned long long rb_entries(const rb_count_table &T, uint32_t nsrcs, uint32_t lane) {
  unsigned long long c = 0;
  for (uint32_t k = 0; k < nsrcs; ++k)  // uniform k: the table is read with scalar loads
    if (lane == k) c = rb_count(T.count[k], T.cap[k]);
  for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o, 64);
  return c;
}

// Message bytes (mark included) of a header's error reply (server.cc:8-67).
__device__ __forceinline__ uint32_t rb_error_bytes(uint32_t action) {
  switch (action) {
    case XDRG_RPC_RPC_MISMATCH:
    case XDRG_RPC_PROG_UNAVAIL:
    case XDRG_RPC_PROC_UNAVAIL:
    case XDRG_RPC_GARBAGE_ARGS:
    case XDRG_RPC_SYSTEM_ERR: return 28;
    case XDRG_RPC_PROG_MISMATCH: return 36;
    case XDRG_RPC_AUTH_ERROR: return 24;
    default: return 0;
  }
}

__device__ __forceinline__ uint64_t rb_incl_scan64(uint64_t x) {
  const uint32_t lane = __lane_id();
  for (int o = 1; o < 64; o <<= 1) {
    const uint64_t y = __shfl_up(x, o, 64);
    if (lane >= static_cast<uint32_t>(o)) x += y;
  }
  return x;
}

__global__ __launch_bounds__(kRbThreads) void k_rb_fill(unsigned long long *__restrict__ owner, uint64_t n) {
  const uint64_t i = static_cast<uint64_t>(blockIdx.x) * kRbThreads + threadIdx.x;
  if (i < n) owner[i] = kRbNoOwner;
}

// n == 0: every entry is unused.
__global__ __launch_bounds__(64) void k_rb_count_entries(const rb_count_table T, uint32_t nsrcs,
                                                         unsigned long long *__restrict__ unused) {
  const unsigned long long c = rb_entries(T, nsrcs, threadIdx.x);
  if (threadIdx.x == 0) *unused = c;
}

// One lane per entry.  The workgroup's source is found by a uniform loop over
// the table (kernel arguments: scalar loads).
__global__ __launch_bounds__(kRbThreads) void k_rb_claim(const xdrg_rpc_hdr *__restrict__ hdrs, uint64_t n,
                                                         const rb_claim_table T, uint32_t nsrcs,
                                                         unsigned long long *__restrict__ owner) {
  uint32_t s = 0;
  for (uint32_t k = 1; k < nsrcs; ++k) s = T.blk[k] <= blockIdx.x ? k : s;
  const rb_claim_src S = T.e[s];
  const uint64_t pos = static_cast<uint64_t>(blockIdx.x - T.blk[s]) * kRbThreads + threadIdx.x;
  if (pos >= rb_count(S.count, S.cap)) return;
  {
    const uint64_t i = S.index[pos];
    if (i < n && hdrs[i].action == XDRG_RPC_DISPATCH) {
      const uint64_t a = S.offsets ? S.offsets[pos] : pos * S.fixed;
      const uint64_t b = S.offsets ? S.offsets[pos + 1] : a + S.fixed;
      if (b >= a && b <= S.bytes_len && !((a | b) & 3u) && b - a <= XDRG_MAX_MSG - 24u)
        atomicMin(owner + i, (static_cast<unsigned long long>(s) << 32) | pos);
    }
  }
}

// The reply of message i: its bytes, and for a success reply where the result
// bytes are (*src; owner decides, the claim has checked the span).
__device__ __forceinline__ uint32_t rb_reply(uint32_t action, unsigned long long own, const rb_span_table &T,
                                             const uint8_t **src) {
  *src = nullptr;
  if (action != XDRG_RPC_DISPATCH) return rb_error_bytes(action);
  if (own == kRbNoOwner) return 0u;  // an asynchronous service that has not answered yet
  const uint32_t s = static_cast<uint32_t>(own >> 32) & (XDRG_RPC_MAX_RESULT_SRCS - 1u);
  const uint64_t pos = own & 0xffffffffull;
  const rb_span_src S = T.e[s];
  const uint64_t a = S.offsets ? S.offsets[pos] : pos * S.fixed;
  const uint64_t b = S.offsets ? S.offsets[pos + 1] : a + S.fixed;
  *src = S.bytes + a;
  return 4u * kRbHdrWords + static_cast<uint32_t>(b - a);
}

__global__ __launch_bounds__(kRbThreads) void k_rb_sizes(const xdrg_rpc_hdr *__restrict__ hdrs, uint64_t n,
                                                         const unsigned long long *__restrict__ owner,
                                                         const rb_span_table T,
                                                         unsigned long long *__restrict__ tile_bytes,
                                                         unsigned long long *__restrict__ tile_won) {
  __shared__ unsigned long long wb[kRbThreads / 64];
  __shared__ uint32_t ww[kRbThreads / 64];
  const uint64_t i = static_cast<uint64_t>(blockIdx.x) * kRbThreads + threadIdx.x;
  unsigned long long t = 0;
  bool won = false;
  if (i < n) {
    const uint32_t action = hdrs[i].action;
    const unsigned long long own = action == XDRG_RPC_DISPATCH ? owner[i] : kRbNoOwner;
    const uint8_t *src;
    t = rb_reply(action, own, T, &src);
    won = own != kRbNoOwner;
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
    for (uint32_t k = 0; k < kRbThreads / 64; ++k) { sb += wb[k]; sw += ww[k]; }
    tile_bytes[blockIdx.x] = sb;
    tile_won[blockIdx.x] = sw;
  }
}

// Exclusive scan in place of the nb tile bytes; the total to offsets[n] and
// status->total_bytes; the entries of every source less the winners to
// *unused.  One workgroup of 1024.
__global__ __launch_bounds__(1024) void k_rb_scan(unsigned long long *__restrict__ tile_bytes,
                                                  const unsigned long long *__restrict__ tile_won, uint64_t nb,
                                                  const rb_count_table T, uint32_t nsrcs,
                                                  uint64_t *__restrict__ total_at, xdrg_status *status,
                                                  unsigned long long *__restrict__ unused) {
  __shared__ unsigned long long wb[16], ww[16];
  const uint32_t tid = threadIdx.x, lane = tid & 63u, wid = tid >> 6;
  unsigned long long carry = 0, won = 0;
  for (uint64_t t0 = 0; t0 < nb; t0 += 1024u) {
    const uint64_t j = t0 + tid;
    const unsigned long long b = j < nb ? tile_bytes[j] : 0ull;
    unsigned long long w = j < nb ? tile_won[j] : 0ull;
    const unsigned long long ib = rb_incl_scan64(b);
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
    const unsigned long long entries = unused ? rb_entries(T, nsrcs, lane) : 0ull;
    if (lane == 0) {
      *total_at = carry;
      status->total_bytes = carry;
      if (unused) *unused = entries - won;
    }
  }
}

// The wave's LDS: byte ends and result pointers of its 64 messages, the
// words each message's reply starts with (kRbMaxWords x 64, one column per
// message: a lane writes its column without bank conflicts) and how many of
// them it uses (7 for a success reply, all of an error reply's).
struct rb_wave_lds {
  unsigned long long end[64];
  const uint8_t *src[64];
  uint32_t w[kRbMaxWords][64];
  uint32_t nw[64];
};

// Word `k` of message `m` of the wave.
__device__ __forceinline__ uint32_t rb_word(const rb_wave_lds &L, uint32_t m, uint64_t k) {
  return k < L.nw[m] ? L.w[k][m] : ld32(L.src[m] + 4u * (k - kRbHdrWords));
}

// The first message of the wave whose end is past `off` (off < end[63]).
__device__ __forceinline__ uint32_t rb_find(const rb_wave_lds &L, uint64_t off) {
  uint32_t lo = 0, hi = 63;
  while (lo < hi) {
    const uint32_t mid = (lo + hi) >> 1;
    if (L.end[mid] > off) hi = mid; else lo = mid + 1;
  }
  return lo;
}

template <int W>
__global__ __launch_bounds__(kRbThreads) void k_rb_emit(const xdrg_rpc_hdr *__restrict__ hdrs, uint64_t n,
                                                        const unsigned long long *__restrict__ owner,
                                                        const rb_span_table T, uint8_t *__restrict__ out,
                                                        uint64_t cap, uint64_t *__restrict__ offsets,
                                                        const unsigned long long *__restrict__ tile_bytes,
                                                        unsigned long long *err) {
  __shared__ unsigned long long wb[kRbThreads / 64];
  __shared__ rb_wave_lds lds[kRbThreads / 64];
  const uint32_t tid = threadIdx.x, lane = tid & 63u, wid = tid >> 6;
  const uint64_t i = static_cast<uint64_t>(blockIdx.x) * kRbThreads + tid;
  rb_wave_lds &L = lds[wid];
  uint32_t bytes = 0, nw = 0;
  const uint8_t *src = nullptr;
  if (i < n) {
    const xdrg_rpc_hdr *h = hdrs + i;
    const u32x4 q = *reinterpret_cast<const u32x4 *>(h);  // xid, action | err | mtype, w[0], w[1]
    const uint32_t action = q.y & 0xffffu;
    const unsigned long long own = action == XDRG_RPC_DISPATCH ? owner[i] : kRbNoOwner;
    bytes = rb_reply(action, own, T, &src);
    if (bytes) {
      // message_t::alloc mark (marshal.cc:15-31), then the xdr_put words
      uint32_t w3 = 0 /* MSG_ACCEPTED */, w4 = 0 /* AUTH_NONE */, w5 = 0 /* body<> */, w6 = 0 /* SUCCESS */;
      uint32_t w7 = 0, w8 = 0;
      if (action == XDRG_RPC_RPC_MISMATCH) {  // rpc_rpc_mismatch_msg, server.cc:55-68
        w3 = 1 /* MSG_DENIED */; w4 = 0 /* RPC_MISMATCH */; w5 = 2; w6 = 2;
      } else if (action == XDRG_RPC_AUTH_ERROR) {  // rpc_auth_error_msg, server.cc:41-53
        w3 = 1 /* MSG_DENIED */; w4 = 1 /* AUTH_ERROR */; w5 = h->w[XDRG_RPC_W_WHY];
      } else if (action != XDRG_RPC_DISPATCH) {  // rpc_accepted_error_msg / rpc_prog_mismatch_msg, server.cc:8-39
        w6 = action == XDRG_RPC_PROG_UNAVAIL  ? 1u
           : action == XDRG_RPC_PROG_MISMATCH ? 2u
           : action == XDRG_RPC_PROC_UNAVAIL  ? 3u
           : action == XDRG_RPC_GARBAGE_ARGS  ? 4u
                                              : 5u /* SYSTEM_ERR */;
        if (action == XDRG_RPC_PROG_MISMATCH) { w7 = h->w[XDRG_RPC_W_LOW]; w8 = h->w[XDRG_RPC_W_HIGH]; }
      }
      nw = action == XDRG_RPC_DISPATCH ? kRbHdrWords : bytes / 4u;
      L.w[0][lane] = mark_word(bytes - 4u);
      L.w[1][lane] = bswap32(q.x);
      L.w[2][lane] = bswap32(1u /* REPLY */);
      L.w[3][lane] = bswap32(w3);
      L.w[4][lane] = bswap32(w4);
      L.w[5][lane] = bswap32(w5);
      L.w[6][lane] = bswap32(w6);
      L.w[7][lane] = bswap32(w7);
      L.w[8][lane] = bswap32(w8);
    }
  }
  const uint64_t ib = rb_incl_scan64(bytes);
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
  // the replies that fit are a prefix of the wave's stretch
  L.end[lane] = rb_incl_scan64(fits ? bytes : 0u);
  L.src[lane] = src;
  L.nw[lane] = nw;
  __syncthreads();
  const uint64_t total = L.end[63];
  uint8_t *base = out + wbase;
  if constexpr (W == 4) {
    for (uint64_t off = 4ull * lane; off < total; off += 256u) {
      const uint32_t m = rb_find(L, off);
      const uint64_t start = m ? L.end[m - 1] : 0u;
      st32(base + off, rb_word(L, m, (off - start) >> 2));
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
      uint32_t m = rb_find(L, first);
      const uint64_t start = m ? L.end[m - 1] : 0u, k0 = (first - start) >> 2;
      if (full && k0 >= L.nw[m] && first + 16u <= L.end[m]) {  // four words of one result
        *reinterpret_cast<u32x4 *>(base + o0) = ld16u(L.src[m] + 4u * (k0 - kRbHdrWords));
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
        v[j] = rb_word(L, m, (o - st) >> 2);
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
