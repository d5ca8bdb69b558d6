// The asynchronous client over many connections (socks.hip): every rpc_sock
// has its own xid_ (xdrpp/msgsock.h:118-122) and its own calls_
// (msgsock.cc:202-232), and abort_all_calls (msgsock.cc:190-200) empties the
// calls_ of the one socket it runs on.  The table is two parallel arrays,
// calls[] and sock[], sorted by (sock, xid as unsigned): the concatenation, in
// socket order, of the tables the single-socket kernels take.  Every kernel
// here finds its socket's run of the table by binary search and then does,
// inside that run, what pending_kernels.h does on any run -- the same
// functions its single-socket sibling calls on a whole table.
//
//   k_sk_next_xids    one lane per xid: its socket's run of the batch and of
//                     the table, then the (k - a + 1)-th value after that
//                     socket's last xid that is not pending there; nsocks more
//                     lanes write every socket's new xid_
//   k_sk_pending_add  one lane per old and per new entry: its place in the
//                     merged table, and the socket it belongs to
//   k_sk_claim / k_pending_resolve   recv_msg for every message, the lookup
//                     keyed by (the socket the message arrived on, word 0)
//   k_sk_call_stats   call_stats with NETWORK_ERROR for an unanswered call of a
//                     closed socket
//   k_sk_count, k_tile_scan<1, 1, count_total>, k_sk_scatter   retire_count and
//                     retire_scatter with the keep rule "no reply and its
//                     socket open", both arrays compacted
//
// No read or write leaves the given arrays, whatever they hold: a lower bound
// is at most its array's length, a socket number indexes last[] and closed[]
// only below nsocks, and every scattered store is compared with its array's
// length first.
#pragma once
#include "pending_kernels.h"

namespace xdrg {
namespace dev {

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

// ------------------------------------------------------------- next xids
// Lanes 0..n-1: call k of the batch, of socket g = call_sock[k], is call k - a
// of g's run [a, b) of the batch and counts on from last[g] over g's run of
// the table.  Lanes n..n+nsocks-1 (last_out only): socket g's xid_ after the
// batch, the xid of its run's last call, computed again (not read back from
// xids: another lane's store).
__global__ __launch_bounds__(kPendingThreads) void k_sk_next_xids(
    const xdrg_rpc_call *__restrict__ calls, const uint32_t *__restrict__ sock, uint64_t ncalls,
    const uint32_t *__restrict__ last, uint64_t nsocks, const uint32_t *__restrict__ call_sock, uint64_t n,
    uint32_t *__restrict__ xids, uint32_t *__restrict__ last_out) {
  const uint64_t t = static_cast<uint64_t>(blockIdx.x) * kPendingThreads + threadIdx.x;
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
  const uint32_t x = pt_nth_free(calls + lo, hi - lo, from, k);
  if (tail) last_out[g] = x; else xids[t] = x;
}

// ----------------------------------------------------------- pending add
// send_call's emplace (msgsock.cc:227-232) for every socket.  With [lo, hi)
// socket g's run of the table and [a, b) its run of the new calls, its part of
// the merged table is [lo + a, hi + b): the sockets before it brought lo old
// and a new entries.  Inside that part an entry lands by the two rules of
// pending_kernels.h ("pending add").
__global__ __launch_bounds__(kPendingThreads) void k_sk_pending_add(
    const xdrg_rpc_call *__restrict__ calls, const uint32_t *__restrict__ sock, uint64_t ncalls,
    const xdrg_rpc_call *__restrict__ fresh, const uint32_t *__restrict__ fresh_sock, uint64_t n,
    xdrg_rpc_call *__restrict__ merged, uint32_t *__restrict__ merged_sock, uint64_t *__restrict__ old_pos,
    uint64_t *__restrict__ new_pos) {
  const uint64_t t = static_cast<uint64_t>(blockIdx.x) * kPendingThreads + threadIdx.x;
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
    w = b > a ? pt_wrap_point(fresh + a, b - a) : 0u;
    lo = sk_below(sock, ncalls, g0), hi = sk_upto(sock, ncalls, g0);
  } else {
    a = sk_below(fresh_sock, n, g), b = sk_upto(fresh_sock, n, g);
    w = b > a ? pt_wrap_point(fresh + a, b - a) : 0u;
    lo = hi = 0u;
    if (!old) lo = sk_below(sock, ncalls, g), hi = sk_upto(sock, ncalls, g);
  }
  uint64_t at;
  if (old) {
    at = t + a + pt_fresh_below(fresh + a, b - a, w, c.xid);
  } else {
    const uint64_t kk = k - a;  // k in [a, b) for a sorted fresh_sock
    const uint64_t rank = kk < w ? ((b - a) - w) + kk : kk - w;
    at = lo + a + pt_lower_bound(calls + lo, hi - lo, c.xid) + rank;
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
// One message per lane, as k_reply_claim, in the calls_ of the socket the
// message arrived on: kUnknownCall also for a REPLY whose row is no row, and
// for one whose xid is pending on another socket.
__global__ __launch_bounds__(kPendingThreads) void k_sk_claim(
    const uint8_t *__restrict__ s, uint64_t len, const uint64_t *__restrict__ offs, uint64_t n,
    const uint32_t *__restrict__ msg_row, const uint32_t *__restrict__ row_sock, uint64_t nrows,
    const xdrg_rpc_call *__restrict__ calls, const uint32_t *__restrict__ sock, uint64_t ncalls,
    unsigned long long *__restrict__ call, unsigned long long *__restrict__ reply_of) {
  const uint64_t i = static_cast<uint64_t>(blockIdx.x) * kPendingThreads + threadIdx.x;
  if (i >= n) return;
  unsigned long long c = kNoCall;
  uint32_t xid = 0u, g = 0u;
  bool look = false;  // a REPLY on a row that is a row
  if (reply_xid(s, len, offs, i, &xid)) {
    c = kUnknownCall;
    const uint32_t row = msg_row[i];
    if (row < nrows) {
      g = row_sock ? row_sock[row] : row;
      look = true;
    }
  }
  if (look) {
    // one socket for all the wave's lookups (one connection's replies): its run once a wave
    uint32_t g0;
    uint64_t lo, hi;
    if (sk_wave_socket(g, &g0)) lo = sk_below(sock, ncalls, g0), hi = sk_upto(sock, ncalls, g0);
    else lo = sk_below(sock, ncalls, g), hi = sk_upto(sock, ncalls, g);
    c = pt_claim(calls, ncalls, lo, hi, xid, i, reply_of);
  }
  call[i] = c;
}

// ------------------------------------------------------------- call stats
// abort_all_calls ran on socket g (msgsock.cc:190-200).  A socket number that
// is no socket counts as open.
__device__ __forceinline__ bool sk_closed(const uint32_t *__restrict__ closed, uint64_t nsocks, uint32_t g) {
  return g < nsocks && closed[g] != 0u;
}

// `unanswered` chosen per entry: NETWORK_ERROR (arpc.h:60-61) for a call still
// outstanding on a closed socket.  A call answered before its socket failed
// keeps its reply's stat: recv_msg had erased it (msgsock.cc:217-219) before
// abort_all_calls ran.
struct sk_unanswered {
  const uint32_t *__restrict__ sock, *__restrict__ closed;
  uint64_t nsocks;
  __device__ __forceinline__ uint32_t operator()(uint64_t c) const {
    return sk_closed(closed, nsocks, sock[c]) ? XDRG_RPCS_NETWORK_ERROR : XDRG_RPCS_PENDING;
  }
};

__global__ __launch_bounds__(kTileThreads) void k_sk_call_stats(const xdrg_rpc_hdr *__restrict__ hdrs, uint64_t n,
                                                              const uint64_t *__restrict__ reply_of,
                                                              const uint32_t *__restrict__ sock, uint64_t ncalls,
                                                              const uint32_t *__restrict__ closed, uint64_t nsocks,
                                                              xdrg_rpc_call_stat *__restrict__ stats) {
  call_stats(hdrs, n, reply_of, ncalls, sk_unanswered{sock, closed, nsocks}, stats);
}

// ---------------------------------------------------------------- retire
// calls_ of every socket after the batch: an entry stays iff no message
// answered it and abort_all_calls did not run on its socket.
struct sk_table {
  const xdrg_rpc_call *__restrict__ calls;
  const uint32_t *__restrict__ sock;
  uint64_t ncalls;
  const uint64_t *__restrict__ reply_of;
  const uint32_t *__restrict__ closed;
  uint64_t nsocks;
  xdrg_rpc_call *__restrict__ kept;
  uint32_t *__restrict__ kept_sock;
  __device__ __forceinline__ bool keep(uint64_t j) const {
    return reply_of[j] == XDRG_RPC_NO_CALL && !sk_closed(closed, nsocks, sock[j]);
  }
  __device__ __forceinline__ void put(uint64_t rank, uint64_t j) const {
    kept[rank] = calls[j];
    kept_sock[rank] = sock[j];
  }
};

__global__ __launch_bounds__(kTileThreads) void k_sk_count(const uint64_t *__restrict__ reply_of,
                                                         const uint32_t *__restrict__ sock, uint64_t ncalls,
                                                         const uint32_t *__restrict__ closed, uint64_t nsocks,
                                                         unsigned long long *__restrict__ tile_kept) {
  retire_count(sk_table{nullptr, sock, ncalls, reply_of, closed, nsocks, nullptr, nullptr}, tile_kept);
}

__global__ __launch_bounds__(kTileThreads) void k_sk_scatter(
    const xdrg_rpc_call *__restrict__ calls, const uint32_t *__restrict__ sock, uint64_t ncalls,
    const uint64_t *__restrict__ reply_of, const uint32_t *__restrict__ closed, uint64_t nsocks,
    const unsigned long long *__restrict__ tile_base, xdrg_rpc_call *__restrict__ kept,
    uint32_t *__restrict__ kept_sock, uint64_t *__restrict__ kept_pos) {
  retire_scatter(sk_table{calls, sock, ncalls, reply_of, closed, nsocks, kept, kept_sock}, tile_base, kept_pos);
}

}  // namespace dev
}  // namespace xdrg
