// The asynchronous client's replies on gfx950: the launchers of
// replies_kernels.h.
//
//   xdrg_rpc_match_replies    rpc_sock::recv_msg (xdrpp/msgsock.cc:202-232)
//                             for every message of a batch: replies in any
//                             order joined to the pending calls by xid, the
//                             first reply to a call wins
//   xdrg_rpc_verify_results   the reply callback of asynchronous_client_base::
//                             invoke (xdrpp/arpc.h:59-90) for every matched
//                             reply, all result types in one launch
//   xdrg_rpc_gather_results   one result type's bytes as a contiguous indexed
//                             stream for xdrg_decode
//
// Every call validates its arguments on the host before the first HIP call,
// launches kernels only (no memset or memcpy nodes: xdrgpu.h "Graph
// capture") and keeps no state.
#include <hip/hip_runtime.h>

#include "plan.h"
#include "replies_kernels.h"

namespace {

using namespace xdrg;
using namespace xdrg::dev;

#define HIPCHK(x)                                                             \
  do {                                                                        \
    hipError_t e_ = (x);                                                      \
    if (e_ != hipSuccess) return xdrg::record_hip_error(int(e_), #x);         \
  } while (0)

// Dynamic LDS a workgroup may ask for without opting in to more.
constexpr size_t kLdsBudget = 48u << 10;

bool misaligned(const void *p, uintptr_t mask) { return reinterpret_cast<uintptr_t>(p) & mask; }

// tile counts, then tile bytes (each nb + 1 u64, 256-byte aligned)
size_t gather_ws_half(uint64_t n) { return (((n + kGatherThreads - 1) / kGatherThreads + 1) * 8 + 255) / 256 * 256; }

}  // namespace

extern "C" {

int xdrg_rpc_match_replies(const void *d_stream, uint64_t len, const uint64_t *d_offsets, uint64_t n,
                           const xdrg_rpc_call *d_calls, uint64_t ncalls, xdrg_rpc_hdr *d_hdrs,
                           uint64_t *d_call, uint64_t *d_reply_of, void *stream) {
  if (n && (!d_offsets || !d_hdrs || !d_call || (!d_stream && len))) return XDRG_EINVAL;
  if (ncalls && (!d_calls || !d_reply_of)) return XDRG_EINVAL;
  if (misaligned(d_stream, 3) || misaligned(d_offsets, 7) || misaligned(d_calls, 7) || misaligned(d_hdrs, 15) ||
      misaligned(d_call, 7) || misaligned(d_reply_of, 7))
    return XDRG_EALIGN;
  if (n == 0 && ncalls == 0) return XDRG_OK;
  const uint64_t nb = (n + kReplyThreads - 1) / kReplyThreads;
  if (nb > 0x7fffffffull || ncalls > 0x7fffffffffffull) return XDRG_EUNSUPPORTED;
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (ncalls) HIPCHK(static_cast<hipError_t>(fill32(d_reply_of, 0xffffffffu, 2 * ncalls, stream)));
  if (n == 0) return XDRG_OK;
  auto *call = reinterpret_cast<unsigned long long *>(d_call);
  auto *reply_of = reinterpret_cast<unsigned long long *>(d_reply_of);
  k_reply_claim<<<uint32_t(nb), kReplyThreads, 0, s>>>(static_cast<const uint8_t *>(d_stream), len, d_offsets, n,
                                                       d_calls, ncalls, call, reply_of);
  HIPCHK(hipGetLastError());
  k_reply_resolve<<<uint32_t(nb), kReplyThreads, 0, s>>>(d_hdrs, n, call, reply_of);
  HIPCHK(hipGetLastError());
  return XDRG_OK;
}

int xdrg_rpc_verify_results(const void *d_stream, uint64_t len, xdrg_rpc_hdr *d_hdrs, const uint64_t *d_call,
                            uint64_t n, const xdrg_rpc_call *d_calls, uint64_t ncalls,
                            const xdrg_plan *const *plans, uint32_t nplans, uint32_t res_base,
                            uint32_t stack_limit, uint32_t *d_verdicts, void *stream) {
  if (nplans > XDRG_RPC_MAX_ARGPLANS || (nplans && !plans)) return XDRG_EINVAL;
  if (n && (!d_hdrs || !d_call || (!d_stream && len) || (ncalls && !d_calls))) return XDRG_EINVAL;
  if (misaligned(d_stream, 3) || misaligned(d_hdrs, 15) || misaligned(d_call, 7) || misaligned(d_calls, 7) ||
      misaligned(d_verdicts, 3))
    return XDRG_EALIGN;
  if (n == 0) return XDRG_OK;
  verify_argtable tab = {};
  bool sub = false;
  size_t ops_lds = 0;
  for (uint32_t i = 0; i < nplans; ++i) {
    if (!plans[i]) continue;  // xdr_void
    const dev_tables *T = nullptr;
    const int rc = plan_tables(plans[i], &T);
    if (rc != XDRG_OK) return rc;
    tab.e[i] = verify_argplan{T->d_ops, T->d_table, uint32_t(plans[i]->ops.size()), 0, 0, 0};
    sub = sub || plans[i]->has_sub;
    ops_lds += plans[i]->ops.size() * sizeof(xdrg_op);
  }
  const uint32_t nt = sub ? kVerifySubThreads : kVerifyThreads;
  const uint64_t nb = (n + nt - 1) / nt;
  if (nb > 0x7fffffffull) return XDRG_EUNSUPPORTED;
  hipStream_t s = static_cast<hipStream_t>(stream);
  const uint8_t *x8 = static_cast<const uint8_t *>(d_stream);
  const auto *call = reinterpret_cast<const unsigned long long *>(d_call);
  const size_t frames = sub ? 4u * verify_frame_words(nt) : 0u;
  const bool lds_ops_fit = ops_lds + frames <= kLdsBudget;  // every plan's ops, staged per workgroup
  const size_t lds = frames + (lds_ops_fit ? ops_lds : 0u);
#define XDRG_VERIFY_RES(SUB, LDSOPS)                                                                          \
  k_rpc_verify_results<SUB, LDSOPS><<<uint32_t(nb), nt, lds, s>>>(x8, len, d_hdrs, call, n, d_calls, ncalls, \
                                                                  tab, nplans, res_base, stack_limit, d_verdicts)
  if (sub) { if (lds_ops_fit) XDRG_VERIFY_RES(true, true); else XDRG_VERIFY_RES(true, false); }
  else { if (lds_ops_fit) XDRG_VERIFY_RES(false, true); else XDRG_VERIFY_RES(false, false); }
#undef XDRG_VERIFY_RES
  HIPCHK(hipGetLastError());
  return XDRG_OK;
}

size_t xdrg_rpc_gather_results_workspace_size(uint64_t n) { return 2 * gather_ws_half(n); }

int xdrg_rpc_gather_results(const void *d_stream, uint64_t len, const xdrg_rpc_hdr *d_hdrs,
                            const uint64_t *d_call, uint64_t n, const xdrg_rpc_call *d_calls, uint64_t ncalls,
                            uint32_t res, uint8_t *d_results, uint64_t results_capacity, uint64_t *d_offsets,
                            uint64_t *d_index, uint64_t *d_count, void *d_workspace, size_t workspace_bytes,
                            xdrg_status *d_status, void *stream) {
  if (!d_offsets || !d_count || !d_status) return XDRG_EINVAL;
  if (n && (!d_hdrs || !d_call || !d_index || (!d_stream && len) || (ncalls && !d_calls))) return XDRG_EINVAL;
  if (!d_results && results_capacity) return XDRG_EINVAL;
  if (misaligned(d_hdrs, 15) || misaligned(d_call, 7) || misaligned(d_calls, 7) || misaligned(d_offsets, 7) ||
      misaligned(d_index, 7) || misaligned(d_count, 7) || misaligned(d_workspace, 7))
    return XDRG_EALIGN;
  if (n == 0) {
    HIPCHK(static_cast<hipError_t>(fill32(d_offsets, 0u, 2, stream)));
    HIPCHK(static_cast<hipError_t>(fill32(d_count, 0u, 2, stream)));
    HIPCHK(static_cast<hipError_t>(fill32(&d_status->total_bytes, 0u, 2, stream)));
    return XDRG_OK;
  }
  if (!d_workspace || workspace_bytes < 2 * gather_ws_half(n)) return XDRG_ESPACE;
  const uint64_t nb = (n + kGatherThreads - 1) / kGatherThreads;
  if (nb > 0x7fffffffull) return XDRG_EUNSUPPORTED;
  hipStream_t s = static_cast<hipStream_t>(stream);
  auto *tcnt = static_cast<unsigned long long *>(d_workspace);
  auto *tbytes = tcnt + gather_ws_half(n) / 8;
  const gather_res_key K{reinterpret_cast<const unsigned long long *>(d_call), d_calls, ncalls, res};
  const uint8_t *x8 = static_cast<const uint8_t *>(d_stream);
  k_gather_res_count<<<uint32_t(nb), kGatherThreads, 0, s>>>(d_hdrs, n, len, K, tcnt, tbytes);
  HIPCHK(hipGetLastError());
  k_gather_scan<<<1, 1024, 0, s>>>(tcnt, tbytes, nb, d_count, d_offsets, d_status);
  HIPCHK(hipGetLastError());
  k_gather_res_emit<<<uint32_t(nb), kGatherThreads, 0, s>>>(
      x8, len, d_hdrs, n, K, d_results, results_capacity, d_offsets, d_index, tcnt, tbytes,
      reinterpret_cast<unsigned long long *>(&d_status->first_error));
  HIPCHK(hipGetLastError());
  return XDRG_OK;
}

}  // extern "C"
