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

#include "pending_host.h"
#include "replies_kernels.h"
#include "verify_host.h"

using namespace xdrg;
using namespace xdrg::dev;
using namespace xdrg::host;

extern "C" {

int xdrg_rpc_match_replies(const void *d_stream, uint64_t len, const uint64_t *d_offsets, uint64_t n,
                           const xdrg_rpc_call *d_calls, uint64_t ncalls, xdrg_rpc_hdr *d_hdrs,
                           uint64_t *d_call, uint64_t *d_reply_of, void *stream) {
  if (n && (!d_offsets || !d_hdrs || !d_call || (!d_stream && len))) return XDRG_EINVAL;
  if (ncalls && (!d_calls || !d_reply_of)) return XDRG_EINVAL;
  if (misaligned(d_stream, 3) || misaligned(d_offsets, 7) || misaligned(d_calls, 7) || misaligned(d_hdrs, 15) ||
      misaligned(d_call, 7) || misaligned(d_reply_of, 7))
    return XDRG_EALIGN;
  return launch_match(n, ncalls, d_hdrs, d_call, d_reply_of, stream,
                      [&](uint32_t nb, hipStream_t s, unsigned long long *call, unsigned long long *reply_of) {
                        k_reply_claim<<<nb, kPendingThreads, 0, s>>>(static_cast<const uint8_t *>(d_stream), len,
                                                                     d_offsets, n, d_calls, ncalls, call, reply_of);
                      });
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
  const verify_geom g = verify_geometry(sub, ops_lds, n);  // every plan's ops, staged per workgroup
  if (g.nb > 0x7fffffffull) return XDRG_EUNSUPPORTED;
  hipStream_t s = static_cast<hipStream_t>(stream);
  const uint8_t *x8 = static_cast<const uint8_t *>(d_stream);
  const auto *call = reinterpret_cast<const unsigned long long *>(d_call);
#define XDRG_VERIFY_RES(SUB, LDSOPS)                                                                     \
  k_rpc_verify_results<SUB, LDSOPS><<<uint32_t(g.nb), g.nt, g.lds, s>>>(x8, len, d_hdrs, call, n, d_calls, \
                                                                        ncalls, tab, nplans, res_base,    \
                                                                        stack_limit, d_verdicts)
  if (sub) { if (g.lds_ops) XDRG_VERIFY_RES(true, true); else XDRG_VERIFY_RES(true, false); }
  else { if (g.lds_ops) XDRG_VERIFY_RES(false, true); else XDRG_VERIFY_RES(false, false); }
#undef XDRG_VERIFY_RES
  HIPCHK(hipGetLastError());
  return XDRG_OK;
}

size_t xdrg_rpc_gather_results_workspace_size(uint64_t n) { return gather_ws_bytes(n); }

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
  const gather_res_key K{reinterpret_cast<const unsigned long long *>(d_call), d_calls, ncalls, res};
  return launch_gather(K, d_stream, len, d_hdrs, n, d_results, results_capacity, d_offsets, d_index, d_count,
                       d_workspace, workspace_bytes, d_status, stream);
}

}  // extern "C"
