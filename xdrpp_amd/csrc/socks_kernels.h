// The asynchronous client over many connections (socks.hip): every rpc_sock
// has its own xid_ (xdrpp/msgsock.h:118-122) and its own calls_
// (msgsock.cc:202-232), and abort_all_calls (msgsock.cc:190-200) empties the
// calls_ of the one socket it runs on.  The table is two parallel arrays,
// calls[] and sock[], sorted by (sock, xid as unsigned): the concatenation, in
// socket order, of the tables the single-socket kernels take
// (call_batch_kernels.h, replies_kernels.h, settle_kernels.h).  Every kernel
// here finds its socket's run of the table by binary search and then does,
// inside that run, exactly what its single-socket sibling does on a whole
// table.
//
//   k_sk_next_xids    one lane per xid: its socket's run of the batch and of
//                     the table, then the (k - a + 1)-th value after that
//                     socket's last xid that is not pending there; nsocks more
//                     lanes write every socket's new xid_
//   k_sk_pending_add  one lane per old and per new entry: its place in the
//                     merged table, and the socket it belongs to
//   k_sk_claim / k_sk_resolve   recv_msg for every message, the lookup keyed
//                     by (the socket the message arrived on, word 0); the
//                     lowest message index claims a call by a 64-bit atomicMin
//   k_sk_call_stats   one lane per entry: rpc_call_stat(hdr), NETWORK_ERROR for
//                     an unanswered call of a closed socket
//   k_sk_count, k_tile_scan<1, 1, count_total>, k_sk_scatter   the ordered
//                     compaction of settle_kernels.h with the keep rule "no
//                     reply and its socket open", both arrays compacted
//
// No read or write leaves the given arrays, whatever they hold: a lower bound
// is at most its array's length, a socket number indexes last[] and closed[]
// only below nsocks, and every scattered store is compared with its array's
// length first.
#pragma once
#include "batch_kernels.h"

namespace xdrg {
namespace dev {

constexpr uint32_t kSkThreads = 256;
constexpr unsigned long long kSkNoCall = XDRG_RPC_NO_CALL;
// d_call between the two match kernels: a REPLY no entry of its socket answers
constexpr unsigned long long kSkUnknown = XDRG_RPC_NO_CALL - 1u;

// ------------------------------------------------------------------ runs
// The elements of the sorted a[0, n) below g, and those not above it.  For any
// array, sorted or not, sk_below(g) <= sk_upto(g) <= n: the two searches
// probe the same places until one probe holds g itself, and part to either
// side of it.
__device__ __forceinline__ uint64_t sk_below(const uint32_t *__restrict__ a, uint64_t n, uint32_t g) {
  uint64_t lo = 0, hi = n;
  while (lo < hi) {
    const uint64_t mid = lo + ((hi - lo) >> 1);
    if (a[mid] < g) lo = mid + 1; else hi = mid;
  }
  return lo;
}
__device__ __forceinline__ uint64_t sk_upto(const uint32_t *__restrict__ a, uint64_t n, uint32_t g) {
  uint64_t lo = 0, hi = n;
  while (lo < hi) {
    const uint64_t mid = lo + ((hi - lo) >> 1);
    if (a[mid] <= g) lo = mid + 1; else hi = mid;
  }
  return lo;
}

// Whether every active lane of the wave holds the same socket number, which
// *g0 then carries as a scalar.  The lanes of a wave mostly share a socket
// (64 neighbours of a batch or a table in socket order), and the searches for
// that socket's runs are the same in every lane: with g0 they are scalar
// loads and scalar arithmetic, done once a wave.  The searches inside the run
// stay per lane.
__device__ __forceinline__ bool sk_wave_socket(uint32_t g, uint32_t *g0) {
  *g0 = __builtin_amdgcn_readfirstlane(g);
  return __ballot(g != *g0) == 0ull;
}

// The entries of a sorted table (one socket's run) whose xid is below x.
__device__ __forceinline__ uint64_t sk_xid_below(const xdrg_rpc_call *__restrict__ calls, uint64_t ncalls,
                                                 uint32_t x) {
  uint64_t lo = 0, hi = ncalls;
  while (lo < hi) {
    const uint64_t mid = lo + ((hi - lo) >> 1);
    if (calls[mid].xid < x) lo = mid + 1; else hi = mid;
  }
  return lo;
}

// ------------------------------------------------------------- next xids
// rpc_sock::get_xid() (msgsock.h:118-122) for the k-th call of one socket,
// every earlier one followed by send_call: the (k+1)-th value after `last`
// that is not in calls[0, ncalls), as k_cb_next_xids finds it (rotated
// coordinates).
__device__ __forceinline__ uint32_t sk_nth_free(const xdrg_rpc_call *__restrict__ calls, uint64_t ncalls,
                                                uint32_t last, uint64_t k) {
  const uint32_t base = last + 1u;
  const uint64_t s = sk_xid_below(calls, ncalls, base);
  uint64_t lo = 0, hi = ncalls;
  while (lo < hi) {
    const uint64_t mid = lo + ((hi - lo) >> 1);
    const uint64_t at = s + mid < ncalls ? s + mid : s + mid - ncalls;
    const uint64_t r = static_cast<uint32_t>(calls[at].xid - base);
    if (static_cast<int64_t>(r) - static_cast<int64_t>(mid) > static_cast<int64_t>(k)) hi = mid; else lo = mid + 1;
  }
  return base + static_cast<uint32_t>(k) + static_cast<uint32_t>(lo);
}

// Lanes 0..n-1: call k of the batch, of socket g = call_sock[k], is call k - a
// of g's run [a, b) of the batch and counts on from last[g] over g's run of
// the table.  Lanes n..n+nsocks-1 (last_out only): socket g's xid_ after the
// batch, the xid of its run's last call, computed again (not read back from
// xids: another lane's store).
__global__ __launch_bounds__(kSkThreads) void k_sk_next_xids(const xdrg_rpc_call *__restrict__ calls,
                                                             const uint32_t *__restrict__ sock, uint64_t ncalls,
                                                             const uint32_t *__restrict__ last, uint64_t nsocks,
                                                             const uint32_t *__restrict__ call_sock, uint64_t n,
                                                             uint32_t *__restrict__ xids,
                                                             uint32_t *__restrict__ last_out) {
  const uint64_t t = static_cast<uint64_t>(blockIdx.x) * kSkThreads + threadIdx.x;
  if (t >= n + (last_out ? nsocks : 0u)) return;
  const bool tail = t >= n;
  const uint32_t g = tail ? static_cast<uint32_t>(t - n) : call_sock[t];
  uint32_t g0, from;
  uint64_t a, lo, hi;
  if (sk_wave_socket(g, &g0)) {
    from = g0 < nsocks ? last[g0] : 0u;
    a = sk_below(call_sock, n, g0);
    lo = sk_below(sock, ncalls, g0);
    hi = sk_upto(sock, ncalls, g0);
  } else {
    from = g < nsocks ? last[g] : 0u;
    a = sk_below(call_sock, n, g);
    lo = sk_below(sock, ncalls, g);
    hi = sk_upto(sock, ncalls, g);
  }
  uint64_t k;
  if (tail) {
    const uint64_t b = sk_upto(call_sock, n, g);
    if (a == b) {
      last_out[g] = from;
      return;
    }
    k = b - 1u - a;
  } else {
    k = t - a;  // an unsorted call_sock: any value, and any xid
  }
  const uint32_t x = sk_nth_free(calls + lo, hi - lo, from, k);
  if (tail) last_out[g] = x; else xids[t] = x;
}

// ----------------------------------------------------------- pending add
// The first entry of a socket's new calls past the wrap: the smallest k with
// xid_k < xid_0 (n when the xids did not wrap; n > 0).
__device__ __forceinline__ uint64_t sk_wrap_point(const xdrg_rpc_call *__restrict__ fresh, uint64_t n) {
  const uint32_t x0 = fresh[0].xid;
  uint64_t lo = 0, hi = n;
  while (lo < hi) {
    const uint64_t mid = lo + ((hi - lo) >> 1);
    if (fresh[mid].xid >= x0) lo = mid + 1; else hi = mid;
  }
  return lo;
}

// send_call's emplace (msgsock.cc:227-232) for every socket.  With [lo, hi)
// socket g's run of the table and [a, b) its run of the new calls, its part of
// the merged table is [lo + a, hi + b): the sockets before it brought lo old
// and a new entries.  Inside that part an entry lands where k_cb_pending_add
// puts it.
__global__ __launch_bounds__(kSkThreads) void k_sk_pending_add(
    const xdrg_rpc_call *__restrict__ calls, const uint32_t *__restrict__ sock, uint64_t ncalls,
    const xdrg_rpc_call *__restrict__ fresh, const uint32_t *__restrict__ fresh_sock, uint64_t n,
    xdrg_rpc_call *__restrict__ merged, uint32_t *__restrict__ merged_sock, uint64_t *__restrict__ old_pos,
    uint64_t *__restrict__ new_pos) {
  const uint64_t t = static_cast<uint64_t>(blockIdx.x) * kSkThreads + threadIdx.x;
  const uint64_t total = ncalls + n;
  if (t >= total) return;
  const bool old = t < ncalls;
  const uint64_t k = old ? 0u : t - ncalls;
  const uint32_t g = old ? sock[t] : fresh_sock[k];
  const xdrg_rpc_call c = old ? calls[t] : fresh[k];
  uint32_t g0;
  uint64_t a, b, w, lo, hi;  // a <= b <= n, w <= b - a, lo <= hi <= ncalls
  if (sk_wave_socket(g, &g0)) {
    a = sk_below(fresh_sock, n, g0), b = sk_upto(fresh_sock, n, g0);
    w = b > a ? sk_wrap_point(fresh + a, b - a) : 0u;
    lo = sk_below(sock, ncalls, g0), hi = sk_upto(sock, ncalls, g0);
  } else {
    a = sk_below(fresh_sock, n, g), b = sk_upto(fresh_sock, n, g);
    w = b > a ? sk_wrap_point(fresh + a, b - a) : 0u;
    lo = hi = 0u;
    if (!old) lo = sk_below(sock, ncalls, g), hi = sk_upto(sock, ncalls, g);
  }
  uint64_t at;
  if (old) {
    // the socket's new entries below it: in the run before the wrap and in the one after
    at = t + a + sk_xid_below(fresh + a, w, c.xid) + sk_xid_below(fresh + a + w, (b - a) - w, c.xid);
  } else {
    const uint64_t kk = k - a;  // k in [a, b) for a sorted fresh_sock
    const uint64_t rank = kk < w ? ((b - a) - w) + kk : kk - w;
    at = lo + a + sk_xid_below(calls + lo, hi - lo, c.xid) + rank;
  }
  const bool put = at < total;  // always, unless fresh_sock is not sorted
  if (put) {
    merged[at] = c;
    merged_sock[at] = g;
  }
  if (old) {
    if (old_pos) old_pos[t] = put ? at : XDRG_RPC_NO_CALL;
  } else {
    if (new_pos) new_pos[k] = put ? at : XDRG_RPC_NO_CALL;
  }
}

// ------------------------------------------------------------------ match
// recv_msg's lookup (msgsock.cc:210-216) in the calls_ of the socket the
// message arrived on: the entry (g, xid) of the table, or ncalls.
__device__ __forceinline__ uint64_t sk_find_call(const xdrg_rpc_call *__restrict__ calls, uint64_t ncalls,
                                                 uint64_t lo, uint64_t hi, uint32_t xid) {
  const uint64_t e = lo + sk_xid_below(calls + lo, hi - lo, xid);
  return e < hi && calls[e].xid == xid ? e : ncalls;
}

// One message per lane, as k_reply_claim: call[i] = the entry it answers
// (claimed for the lowest i by atomicMin), kSkUnknown for a REPLY no entry of
// its socket answers -- also one whose row is no row, and one whose xid is
// pending on another socket -- and kSkNoCall for everything that is no REPLY.
// reply_of[] was filled with kSkNoCall by the launch before this one.
__global__ __launch_bounds__(kSkThreads) void k_sk_claim(
    const uint8_t *__restrict__ s, uint64_t len, const uint64_t *__restrict__ offs, uint64_t n,
    const uint32_t *__restrict__ msg_row, const uint32_t *__restrict__ row_sock, uint64_t nrows,
    const xdrg_rpc_call *__restrict__ calls, const uint32_t *__restrict__ sock, uint64_t ncalls,
    unsigned long long *__restrict__ call, unsigned long long *__restrict__ reply_of) {
  const uint64_t i = static_cast<uint64_t>(blockIdx.x) * kSkThreads + threadIdx.x;
  if (i >= n) return;
  const uint64_t m0 = offs[i], m1 = offs[i + 1];
  unsigned long long c = kSkNoCall;
  uint32_t xid = 0u, g = 0u;
  bool look = false;  // a REPLY on a row that is a row
  if (m1 <= len && m1 >= m0 && m1 - m0 >= 12u && !(m0 & 3u)) {
    xid = bswap32(ld32(s + m0 + 4));
    if (bswap32(ld32(s + m0 + 8)) == 1u) {  // msg_type REPLY (rpc_msg.x)
      c = kSkUnknown;
      const uint32_t row = msg_row[i];
      if (row < nrows) {
        g = row_sock ? row_sock[row] : row;
        look = true;
      }
    }
  }
  if (look) {
    // one socket for all the wave's lookups (one connection's replies): its run once a wave
    uint32_t g0;
    uint64_t lo, hi;
    if (sk_wave_socket(g, &g0)) lo = sk_below(sock, ncalls, g0), hi = sk_upto(sock, ncalls, g0);
    else lo = sk_below(sock, ncalls, g), hi = sk_upto(sock, ncalls, g);
    const uint64_t e = sk_find_call(calls, ncalls, lo, hi, xid);
    if (e < ncalls) {
      c = e;
      atomicMin(reply_of + e, static_cast<unsigned long long>(i));
    }
  }
  call[i] = c;
}

// The compare, as k_reply_resolve: message i keeps entry c when it is the one
// that claimed it; every other REPLY becomes XDRG_RPCR_UNKNOWN_XID
// ("ignoring reply to unknown call", msgsock.cc:212-216).  A header is
// rewritten through its first 16 bytes (action: the low half of word 1).
__global__ __launch_bounds__(kSkThreads) void k_sk_resolve(xdrg_rpc_hdr *__restrict__ hdrs, uint64_t n,
                                                           unsigned long long *__restrict__ call,
                                                           const unsigned long long *__restrict__ reply_of) {
  const uint64_t i = static_cast<uint64_t>(blockIdx.x) * kSkThreads + threadIdx.x;
  if (i >= n) return;
  const unsigned long long c = call[i];
  if (c == kSkNoCall) return;
  if (c != kSkUnknown && reply_of[c] == i) return;  // the call's first reply
  u32x4 *hp = reinterpret_cast<u32x4 *>(hdrs + i);
  u32x4 q = *hp;
  q.y = (q.y & 0xffff0000u) | XDRG_RPCR_UNKNOWN_XID;  // err and mtype stay
  *hp = q;
  call[i] = kSkNoCall;
}

// ------------------------------------------------------------- call stats
// abort_all_calls ran on socket g (msgsock.cc:190-200).  A socket number that
// is no socket counts as open.
__device__ __forceinline__ bool sk_closed(const uint32_t *__restrict__ closed, uint64_t nsocks, uint32_t g) {
  return g < nsocks && closed[g] != 0u;
}

// k_st_call_stats with `unanswered` chosen per entry: NETWORK_ERROR
// (arpc.h:60-61) for a call still outstanding on a closed socket.  A call
// answered before its socket failed keeps its reply's stat: recv_msg had
// erased it (msgsock.cc:217-219) before abort_all_calls ran.
__global__ __launch_bounds__(kTileThreads) void k_sk_call_stats(const xdrg_rpc_hdr *__restrict__ hdrs, uint64_t n,
                                                              const uint64_t *__restrict__ reply_of,
                                                              const uint32_t *__restrict__ sock, uint64_t ncalls,
                                                              const uint32_t *__restrict__ closed, uint64_t nsocks,
                                                              xdrg_rpc_call_stat *__restrict__ stats) {
  const uint64_t c = static_cast<uint64_t>(blockIdx.x) * kTileThreads + threadIdx.x;
  if (c >= ncalls) return;
  const uint64_t i = reply_of[c];
  xdrg_rpc_call_stat s = {XDRG_RPCS_GARBAGE_RES, 0u};
  if (i == XDRG_RPC_NO_CALL) {
    s.type = sk_closed(closed, nsocks, sock[c]) ? XDRG_RPCS_NETWORK_ERROR : XDRG_RPCS_PENDING;
  } else if (i < n) {
    const xdrg_rpc_hdr &h = hdrs[i];
    const uint32_t a = h.action;
    if (a == XDRG_RPCR_OK) {
      s.type = XDRG_RPCS_ACCEPT_STAT;
    } else if (a == XDRG_RPCR_ACCEPT_STAT) {
      s.type = XDRG_RPCS_ACCEPT_STAT;
      s.stat = h.w[XDRG_RPC_W_STAT];
    } else if (a == XDRG_RPCR_AUTH_STAT) {
      s.type = XDRG_RPCS_AUTH_STAT;
      s.stat = h.w[XDRG_RPC_W_WHY];
    } else if (a == XDRG_RPCR_RPCVERS_MISMATCH) {
      s.type = XDRG_RPCS_RPCVERS_MISMATCH;
    }
  }
  stats[c] = s;
}

// ---------------------------------------------------------------- retire
// calls_ of every socket after the batch: an entry stays iff no message
// answered it and abort_all_calls did not run on its socket.
__device__ __forceinline__ bool sk_keep(const uint64_t *__restrict__ reply_of, const uint32_t *__restrict__ sock,
                                        uint64_t ncalls, const uint32_t *__restrict__ closed, uint64_t nsocks,
                                        uint64_t j) {
  return j < ncalls && reply_of[j] == XDRG_RPC_NO_CALL && !sk_closed(closed, nsocks, sock[j]);
}

__global__ __launch_bounds__(kTileThreads) void k_sk_count(const uint64_t *__restrict__ reply_of,
                                                         const uint32_t *__restrict__ sock, uint64_t ncalls,
                                                         const uint32_t *__restrict__ closed, uint64_t nsocks,
                                                         unsigned long long *__restrict__ tile_kept) {
  const uint64_t j = static_cast<uint64_t>(blockIdx.x) * kTileThreads + threadIdx.x;
  tile_reduce(0, sk_keep(reply_of, sock, ncalls, closed, nsocks, j), nullptr, tile_kept);
}

// As k_st_scatter: a kept entry's rank is at most its own position, and the
// compare keeps every store below ncalls even when the inputs change between
// the passes.
__global__ __launch_bounds__(kTileThreads) void k_sk_scatter(
    const xdrg_rpc_call *__restrict__ calls, const uint32_t *__restrict__ sock, uint64_t ncalls,
    const uint64_t *__restrict__ reply_of, const uint32_t *__restrict__ closed, uint64_t nsocks,
    const unsigned long long *__restrict__ tile_base, xdrg_rpc_call *__restrict__ kept,
    uint32_t *__restrict__ kept_sock, uint64_t *__restrict__ kept_pos) {
  __shared__ uint32_t wk[kTileThreads / 64];
  const uint32_t tid = threadIdx.x, lane = tid & 63u, wid = tid >> 6;
  const uint64_t j = static_cast<uint64_t>(blockIdx.x) * kTileThreads + tid;
  const bool keep = sk_keep(reply_of, sock, ncalls, closed, nsocks, j);
  const unsigned long long m = __ballot(keep);
  if (lane == 0u) wk[wid] = __popcll(m);
  __syncthreads();
  uint64_t rank = tile_base[blockIdx.x] + __popcll(m & ((1ull << lane) - 1ull));
  for (uint32_t k = 0; k < wid; ++k) rank += wk[k];
  if (j >= ncalls) return;
  const bool put = keep && rank < ncalls;
  if (put) {
    kept[rank] = calls[j];
    kept_sock[rank] = sock[j];
  }
  if (kept_pos) kept_pos[j] = put ? rank : XDRG_RPC_NO_CALL;
}

}  // namespace dev
}  // namespace xdrg
