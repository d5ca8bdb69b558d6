// The pending table, rpc_sock::calls_ (xdrpp/msgsock.h, msgsock.cc:202-232),
// as the asynchronous client's stages use it: a run of xdrg_rpc_call sorted by
// xid as unsigned.  For one rpc_sock (call_batch_kernels.h, replies_kernels.h,
// settle.hip) the run is the whole table and its scalars are kernel arguments;
// for many (socks_kernels.h) it is the run of one socket, found by binary
// search.  What is done inside a run lives here, once:
//
//   pt_lower_bound, pt_nth_free     get_xid(): the k-th value after `last`
//                                   that is not pending
//   pt_wrap_point, pt_fresh_below   send_call's emplace: where an old and a
//                                   new entry land in the merge
//   reply_xid, pt_find_call, pt_claim   recv_msg: a REPLY's xid, its entry, the
//                                   64-bit atomicMin by which the lowest
//                                   message index claims it
//   k_pending_resolve               the winner keeps its header, every other
//                                   REPLY becomes XDRG_RPCR_UNKNOWN_XID
//   call_stats<UNANSWERED>          one lane per entry: rpc_call_stat(hdr)
//                                   (k_st_call_stats here)
//   retire_count<T>, k_tile_scan<1, 1, count_total>, retire_scatter<T>
//                                   calls_ after the erases, an ordered
//                                   compaction: a kept entry's rank is the kept
//                                   lanes below it in its wave's ballot, plus
//                                   the waves before it in the tile (LDS), plus
//                                   the tile's base.  T says which entries stay
//                                   and which arrays are compacted
//                                   (k_st_count, k_st_scatter here).
//
// The stats and the retire are device functions, and a kernel hands them its
// own arguments: with the struct itself as the kernel argument the compiler
// fetches its fields in wider scalar loads and the many-socket scatter is six
// instructions longer.
//
// No read or write leaves the given arrays, whatever they hold: a lower bound
// is at most its array's length, and every scattered store is compared with
// its array's length first.  The retire and the stats use no atomic: the order
// is the table's, and the result is a function of the inputs only.
//
// The kernels are templates, so every translation unit that launches one
// links its own instance.
#pragma once
#include "batch_kernels.h"

namespace xdrg {
namespace dev {

constexpr uint32_t kPendingThreads = 256;
constexpr unsigned long long kNoCall = XDRG_RPC_NO_CALL;
// d_call between the two match kernels: a REPLY no entry of its run answers
constexpr unsigned long long kUnknownCall = XDRG_RPC_NO_CALL - 1u;
constexpr uint32_t kMsgReply = 1;  // msg_type REPLY (rpc_msg.x)

// The first 16 bytes of a header (xid, action | err | mtype, w[0], w[1]):
// action in the low half of word 1, err in bits 16-23.  A header is rewritten
// through them: one 16-byte load, one 16-byte store when it changes.
__device__ __forceinline__ uint32_t hdr_action(const u32x4 &q) { return q.y & 0xffffu; }
__device__ __forceinline__ uint32_t hdr_err(const u32x4 &q) { return (q.y >> 16) & 0xffu; }
__device__ __forceinline__ void hdr_set(u32x4 &q, uint32_t action, uint32_t err) {
  q.y = (q.y & 0xff000000u) | ((err & 0xffu) << 16) | action;
}
__device__ __forceinline__ u32x4 *hdr_head(xdrg_rpc_hdr *h) { return reinterpret_cast<u32x4 *>(h); }

// ------------------------------------------------------------- next xids
// The entries of calls[0, n) whose xid is below x.
__device__ __forceinline__ uint64_t pt_lower_bound(const xdrg_rpc_call *__restrict__ calls, uint64_t n, uint32_t x) {
  uint64_t lo = 0, hi = n;
  while (lo < hi) {
    const uint64_t mid = lo + ((hi - lo) >> 1);
    if (calls[mid].xid < x) lo = mid + 1; else hi = mid;
  }
  return lo;
}

// rpc_sock::get_xid() (msgsock.h:118-122) for the k-th call of a batch, every
// earlier one followed by send_call: the (k+1)-th value after `last` that is
// not in calls[0, n).  In rotated coordinates r(x) = (x - last - 1) mod 2^32
// the table, read from its split point s = lower_bound(last + 1) on and around
// its end, is ascending: R[0] < R[1] < ...  The k-th free value is k + j for
// the smallest j with R[j] - j > k (j pending values lie at or below it);
// j = n when there is none.  n + the batch <= 2^32 - 1, so the value exists.
__device__ __forceinline__ uint32_t pt_nth_free(const xdrg_rpc_call *__restrict__ calls, uint64_t n, uint32_t last,
                                                uint64_t k) {
  const uint32_t base = last + 1u;
  const uint64_t s = pt_lower_bound(calls, n, base);
  uint64_t lo = 0, hi = n;
  while (lo < hi) {
    const uint64_t mid = lo + ((hi - lo) >> 1);
    const uint64_t at = s + mid < n ? s + mid : s + mid - n;
    const uint64_t r = static_cast<uint32_t>(calls[at].xid - base);
    // r >= mid in a table that keeps the contract; a signed compare keeps a
    // broken one from wrapping
    if (static_cast<int64_t>(r) - static_cast<int64_t>(mid) > static_cast<int64_t>(k)) hi = mid; else lo = mid + 1;
  }
  return base + static_cast<uint32_t>(k) + static_cast<uint32_t>(lo);
}

// ----------------------------------------------------------- pending add
// The first of the n > 0 fresh calls past the wrap: the smallest k with
// xid_k < xid_0 (n when the xids did not wrap).
__device__ __forceinline__ uint64_t pt_wrap_point(const xdrg_rpc_call *__restrict__ fresh, uint64_t n) {
  const uint32_t x0 = fresh[0].xid;
  uint64_t lo = 0, hi = n;
  while (lo < hi) {
    const uint64_t mid = lo + ((hi - lo) >> 1);
    if (fresh[mid].xid >= x0) lo = mid + 1; else hi = mid;
  }
  return lo;
}

// calls_ after the sends (msgsock.cc:227-232), fresh[0, n) with wrap point w
// merged into calls[0, ncalls).  An old entry moves up by the fresh entries
// below it, in the run before the wrap and in the one after.
__device__ __forceinline__ uint64_t pt_fresh_below(const xdrg_rpc_call *__restrict__ fresh, uint64_t n, uint64_t w,
                                                   uint32_t xid) {
  return pt_lower_bound(fresh, w, xid) + pt_lower_bound(fresh + w, n - w, xid);
}
// Fresh entry k lands after the old entries below it, at its rank around the
// wrap: pt_lower_bound(calls, ncalls, xid) + (k < w ? (n - w) + k : k - w), at
// most ncalls + n - 1 for k < n whatever the arrays hold.  The two kernels
// write this sum out: behind a helper the many-socket kernel keeps two more
// VGPRs live.

// ------------------------------------------------------------------ match
// Whether message i, bytes [offs[i], offs[i + 1]) of s, is a REPLY, and its
// xid.  A message shorter than xid + msg_type, a CALL, another msg_type, or
// offsets that are no message of this stream (never read) is none.
__device__ __forceinline__ bool reply_xid(const uint8_t *__restrict__ s, uint64_t len,
                                          const uint64_t *__restrict__ offs, uint64_t i, uint32_t *xid) {
  const uint64_t m0 = offs[i], m1 = offs[i + 1];
  if (!(m1 <= len && m1 >= m0 && m1 - m0 >= 12u && !(m0 & 3u))) return false;
  *xid = bswap32(ld32(s + m0 + 4));
  return bswap32(ld32(s + m0 + 8)) == kMsgReply;
}

// recv_msg's lookup (msgsock.cc:210-216) in the run [lo, hi) of the table: the
// entry with this xid, or ncalls.  Stays inside the run whatever it holds.
__device__ __forceinline__ uint64_t pt_find_call(const xdrg_rpc_call *__restrict__ calls, uint64_t ncalls,
                                                 uint64_t lo, uint64_t hi, uint32_t xid) {
  const uint64_t e = lo + pt_lower_bound(calls + lo, hi - lo, xid);
  return e < hi && calls[e].xid == xid ? e : ncalls;
}

// What call[i] gets for REPLY i with this xid: the entry of the run it answers,
// claimed for the lowest i (msgsock.cc:217-219 erases the call at its first
// reply), or kUnknownCall.  reply_of[] was filled with kNoCall by the launch
// before.
__device__ __forceinline__ unsigned long long pt_claim(const xdrg_rpc_call *__restrict__ calls, uint64_t ncalls,
                                                       uint64_t lo, uint64_t hi, uint32_t xid, uint64_t i,
                                                       unsigned long long *__restrict__ reply_of) {
  const uint64_t e = pt_find_call(calls, ncalls, lo, hi, xid);
  if (e >= ncalls) return kUnknownCall;
  atomicMin(reply_of + e, static_cast<unsigned long long>(i));
  return e;
}

// The compare: message i keeps entry c when it is the one that claimed it;
// every other REPLY becomes XDRG_RPCR_UNKNOWN_XID ("ignoring reply to unknown
// call", msgsock.cc:212-216).  The outcome is a function of the inputs alone.
template <class = void>
__global__ __launch_bounds__(kPendingThreads) void k_pending_resolve(xdrg_rpc_hdr *__restrict__ hdrs, uint64_t n,
                                                                     unsigned long long *__restrict__ call,
                                                                     const unsigned long long *__restrict__ reply_of) {
  const uint64_t i = static_cast<uint64_t>(blockIdx.x) * kPendingThreads + threadIdx.x;
  if (i >= n) return;
  const unsigned long long c = call[i];
  if (c == kNoCall) return;
  if (c != kUnknownCall && reply_of[c] == i) return;  // the call's first reply
  u32x4 *hp = hdr_head(hdrs + i);
  u32x4 q = *hp;
  hdr_set(q, XDRG_RPCR_UNKNOWN_XID, hdr_err(q));
  *hp = q;
  call[i] = kNoCall;
}

// ------------------------------------------------------------- call stats
// rpc_call_stat(hdr) (rpc_msg.cc:69-90) after xdrg_rpc_verify_results, one
// lane per entry: every action a matched reply cannot carry is GARBAGE_RES, as
// is a reply_of that names no message of this batch (no header is read for
// it).  unanswered(c): the type of an entry no message answered.
template <class UNANSWERED>
__device__ __forceinline__ void call_stats(const xdrg_rpc_hdr *__restrict__ hdrs, uint64_t n,
                                           const uint64_t *__restrict__ reply_of, uint64_t ncalls,
                                           const UNANSWERED &unanswered, xdrg_rpc_call_stat *__restrict__ stats) {
  const uint64_t c = static_cast<uint64_t>(blockIdx.x) * kTileThreads + threadIdx.x;
  if (c >= ncalls) return;
  const uint64_t i = reply_of[c];
  xdrg_rpc_call_stat s = {XDRG_RPCS_GARBAGE_RES, 0u};
  if (i == XDRG_RPC_NO_CALL) {
    s.type = unanswered(c);
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

// One rpc_sock: PENDING, or NETWORK_ERROR from abort_all_calls
// (msgsock.cc:190-200, arpc.h:60-61), for every unanswered entry alike.
struct one_unanswered {
  uint32_t type;
  __device__ __forceinline__ uint32_t operator()(uint64_t) const { return type; }
};

template <class = void>
__global__ __launch_bounds__(kTileThreads) void k_st_call_stats(const xdrg_rpc_hdr *__restrict__ hdrs, uint64_t n,
                                                              const uint64_t *__restrict__ reply_of,
                                                              uint64_t ncalls, uint32_t unanswered,
                                                              xdrg_rpc_call_stat *__restrict__ stats) {
  call_stats(hdrs, n, reply_of, ncalls, one_unanswered{unanswered}, stats);
}

// ---------------------------------------------------------------- retire
// T: ncalls, keep(j) for j < ncalls, put(rank, j).  Every lane of the
// kTileThreads must call.
template <class T>
__device__ __forceinline__ void retire_count(const T &table, unsigned long long *__restrict__ tile_kept) {
  const uint64_t j = static_cast<uint64_t>(blockIdx.x) * kTileThreads + threadIdx.x;
  tile_reduce(0, j < table.ncalls && table.keep(j), nullptr, tile_kept);
}

// A kept entry's rank is at most its own position (the entries before it that
// are kept), so every store stays below ncalls; the compare keeps it there
// even when the inputs change between the passes.
template <class T>
__device__ __forceinline__ void retire_scatter(const T &table, const unsigned long long *__restrict__ tile_base,
                                               uint64_t *__restrict__ kept_pos) {
  __shared__ uint32_t wk[kTileThreads / 64];
  const uint32_t tid = threadIdx.x, lane = tid & 63u, wid = tid >> 6;
  const uint64_t j = static_cast<uint64_t>(blockIdx.x) * kTileThreads + tid;
  const bool keep = j < table.ncalls && table.keep(j);
  const unsigned long long m = __ballot(keep);
  if (lane == 0u) wk[wid] = __popcll(m);
  __syncthreads();
  uint64_t rank = tile_base[blockIdx.x] + __popcll(m & ((1ull << lane) - 1ull));
  for (uint32_t k = 0; k < wid; ++k) rank += wk[k];
  if (j >= table.ncalls) return;
  const bool put = keep && rank < table.ncalls;
  if (put) table.put(rank, j);
  if (kept_pos) kept_pos[j] = put ? rank : XDRG_RPC_NO_CALL;
}

// One rpc_sock: an entry stays iff no message answered it.
struct one_table {
  const xdrg_rpc_call *__restrict__ calls;
  uint64_t ncalls;
  const uint64_t *__restrict__ reply_of;
  xdrg_rpc_call *__restrict__ kept;
  __device__ __forceinline__ bool keep(uint64_t j) const { return reply_of[j] == XDRG_RPC_NO_CALL; }
  __device__ __forceinline__ void put(uint64_t rank, uint64_t j) const { kept[rank] = calls[j]; }
};

template <class = void>
__global__ __launch_bounds__(kTileThreads) void k_st_count(const uint64_t *__restrict__ reply_of, uint64_t ncalls,
                                                         unsigned long long *__restrict__ tile_kept) {
  retire_count(one_table{nullptr, ncalls, reply_of, nullptr}, tile_kept);
}

template <class = void>
__global__ __launch_bounds__(kTileThreads) void k_st_scatter(const xdrg_rpc_call *__restrict__ calls, uint64_t ncalls,
                                                           const uint64_t *__restrict__ reply_of,
                                                           const unsigned long long *__restrict__ tile_base,
                                                           xdrg_rpc_call *__restrict__ kept,
                                                           uint64_t *__restrict__ kept_pos) {
  retire_scatter(one_table{calls, ncalls, reply_of, kept}, tile_base, kept_pos);
}

}  // namespace dev
}  // namespace xdrg
