// The asynchronous client's reply step for a whole batch (replies.hip):
// asynchronous_client_base::invoke over rpc_sock (xdrpp/arpc.h:41-91,
// xdrpp/msgsock.cc:202-232) -- every reply is matched to its pending call by
// xid, its result verified with that call's result type, and the results of
// one type gathered for xdrg_decode.
//
//   k_reply_claim / k_pending_resolve   rpc_sock::recv_msg for every message
//       (the steps are pending_kernels.h's, here on the whole table):
//       the message's own xid (word 0) and msg_type (word 1) are read, a
//       REPLY's xid is looked up in the pending table (sorted by xid,
//       unsigned: rpc_sock::calls_) by binary search, and the lowest message
//       index that answers a call claims it with a 64-bit atomicMin
//       (msgsock.cc:217-219 erases the call at its first reply); the second
//       kernel compares: the winner keeps its header, every other reply to
//       the call, and every reply to no call, becomes XDRG_RPCR_UNKNOWN_XID
//       (msgsock.cc:212-216).  The outcome is a function of the inputs alone.
//   k_rpc_verify_results   the reply callback of arpc.h:59-90, one matched
//       reply per lane, each with its call's result plan: archive(g, *res),
//       g.done(), and GARBAGE_RES for the reply that throws (arpc.h:87-89).
//   gather_res_key   one result type's bytes as an indexed stream: the
//       selector of verify_kernels.h's k_gather_count / k_gather_emit.
#pragma once
#include "pending_kernels.h"
#include "verify_kernels.h"

namespace xdrg {
namespace dev {

// One message per lane.  call[i] = the entry its xid names (claimed for the
// lowest i by atomicMin), kUnknownCall for a REPLY to no entry, kNoCall for
// everything that is no REPLY.  reply_of[] was filled with kNoCall by the
// launch before this one.
__global__ __launch_bounds__(kPendingThreads) void k_reply_claim(
    const uint8_t *__restrict__ s, uint64_t len, const uint64_t *__restrict__ offs, uint64_t n,
    const xdrg_rpc_call *__restrict__ calls, uint64_t ncalls, unsigned long long *__restrict__ call,
    unsigned long long *__restrict__ reply_of) {
  const uint64_t i = static_cast<uint64_t>(blockIdx.x) * kPendingThreads + threadIdx.x;
  if (i >= n) return;
  uint32_t xid;
  call[i] = reply_xid(s, len, offs, i, &xid) ? pt_claim(calls, ncalls, 0u, ncalls, xid, i, reply_of) : kNoCall;
}

// ------------------------------------------------------- result verdicts
// The span rules of verify_span for a void result (xdr_void: no bytes), then
// g.done().
__device__ __forceinline__ uint32_t verify_void(uint64_t len, uint64_t a, uint64_t b) {
  if (b < a || b > len || (a & 3u)) return verdict_of(0, XDRG_ERR_OVERFLOW_GET);
  if ((b - a) & 3u) return verdict_of(kOpRecordLevel, XDRG_ERR_SIZE_NOT_MULT4);
  return b > a ? verdict_of(kOpRecordLevel, XDRG_ERR_TRAILING) : 0u;
}

// One header per lane.  T.e[k] serves the calls with res == res_base + k
// (ops == nullptr: a void result; prog, vers and proc are not used).  The
// table is searched by a wave-uniform loop, as in k_rpc_verify_args, and the
// ops are staged the same way.
template <bool SUB, bool LDSOPS>
__global__ __launch_bounds__(SUB ? kVerifySubThreads : kVerifyThreads) void k_rpc_verify_results(
    const uint8_t *__restrict__ xdr, uint64_t len, xdrg_rpc_hdr *__restrict__ hdrs,
    const unsigned long long *__restrict__ call, uint64_t n, const xdrg_rpc_call *__restrict__ calls,
    uint64_t ncalls, const verify_argtable T, uint32_t nplans, uint32_t res_base, uint32_t stack_limit,
    uint32_t *__restrict__ verdicts) {
  extern __shared__ __attribute__((aligned(16))) uint32_t vsm[];
  uint32_t *fbase = vsm;
  if constexpr (LDSOPS) {
    uint32_t at = 0;
    for (uint32_t i = 0; i < nplans; ++i) {
      const uint32_t *src = reinterpret_cast<const uint32_t *>(T.e[i].ops);
      for (uint32_t k = threadIdx.x; k < 8u * T.e[i].nops; k += blockDim.x) vsm[8u * at + k] = src[k];
      at += T.e[i].nops;
    }
    fbase = vsm + 8u * at;
    __syncthreads();
  }
  const uint64_t r = static_cast<uint64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
  if (r >= n) return;
  uint32_t v = 0;
  const unsigned long long c = call[r];
  const uint32_t k = c < ncalls ? calls[c].res - res_base : nplans;
  if (k < nplans) {
    u32x4 *hp = hdr_head(hdrs + r);
    u32x4 q = *hp;
    const uint32_t action = hdr_action(q);
    const uint64_t a = hdrs[r].body_off, b = hdrs[r].end;
    uint32_t err = 0;
    if (action == XDRG_RPCR_OK) {  // archive(g, *res); g.done()  (arpc.h:67-69)
      const xdrg_op *ops = nullptr;
      const uint32_t *table = nullptr;
      uint32_t at = 0;
      for (uint32_t i = 0; i < nplans; ++i) {
        const bool hit = i == k && T.e[i].ops != nullptr;
        ops = hit ? (LDSOPS ? reinterpret_cast<const xdrg_op *>(vsm) + at : T.e[i].ops) : ops;
        table = hit ? T.e[i].table : table;
        at += T.e[i].nops;
      }
      if (ops) {
        using OPS = typename std::conditional<LDSOPS, lds_ops, glob_ops>::type;
        const OPS O{ops};
        if constexpr (SUB) {
          lds_frames fr{fbase + threadIdx.x, blockDim.x};
          v = verify_span(O, table, xdr, len, a, b, stack_limit, fr);
        } else {
          no_frames fr;
          v = verify_span(O, table, xdr, len, a, b, stack_limit, fr);
        }
      } else {
        v = verify_void(len, a, b);
      }
      err = v & 0xffu;
    } else if (action == XDRG_RPCR_ACCEPT_STAT || action == XDRG_RPCR_AUTH_STAT ||
               action == XDRG_RPCR_RPCVERS_MISMATCH) {  // no result, g.done() still runs
      if (b != a) v = verdict_of(kOpRecordLevel, XDRG_ERR_TRAILING);
      err = v & 0xffu;
    } else if (action == XDRG_RPCR_MALFORMED) {  // archive(g, hdr) threw
      err = hdr_err(q);
      v = verdict_of(kOpRecordLevel, err);
    }
    if (v || action == XDRG_RPCR_MALFORMED) {  // cb(rpc_call_stat::GARBAGE_RES), arpc.h:87-89
      hdr_set(q, XDRG_RPCR_GARBAGE_RES, err);
      *hp = q;
    }
  }
  if (verdicts) verdicts[r] = v;
}

// ---------------------------------------------------------- result gather
// The results of one type (the gather of verify_kernels.h with this
// selector): a matched reply that is still OK, of a call with this result
// type.
struct gather_res_key {
  const unsigned long long *call;
  const xdrg_rpc_call *calls;
  uint64_t ncalls;
  uint32_t res;
  __device__ __forceinline__ bool operator()(const xdrg_rpc_hdr *h, uint64_t i) const {
    if (h->action != XDRG_RPCR_OK) return false;
    const unsigned long long c = call[i];
    return c < ncalls && calls[c].res == res;
  }
};

}  // namespace dev
}  // namespace xdrg
