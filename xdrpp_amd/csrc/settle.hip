// Settling a reply batch on gfx950: what the asynchronous client's pending
// calls became, and calls_ after the erases (the kernels are
// pending_kernels.h's, on one rpc_sock's whole table).
//
//   xdrg_rpc_call_stats      the call_result the callback of
//                            asynchronous_client_base::invoke receives for
//                            every pending call: rpc_call_stat(hdr)
//                            (xdrpp/rpc_msg.cc:69-90), GARBAGE_RES for the
//                            reply that threw (arpc.h:87-89), NETWORK_ERROR
//                            from abort_all_calls (msgsock.cc:190-200,
//                            arpc.h:60-61)
//   xdrg_rpc_pending_retire  rpc_sock::calls_ after recv_msg's erases
//                            (xdrpp/msgsock.cc:217-219): an ordered stream
//                            compaction, count -> scan -> scatter
//
// Both validate on the host before the first HIP call, launch kernels only
// (no memset or memcpy nodes: xdrgpu.h "Graph capture") and keep no state.
#include <hip/hip_runtime.h>

#include "pending_host.h"

namespace {

using namespace xdrg;
using namespace xdrg::dev;
using namespace xdrg::host;

static_assert(sizeof(xdrg_rpc_call_stat) == 8, "xdrg_rpc_call_stat is 8 bytes");

}  // namespace

extern "C" {

int xdrg_rpc_call_stats(const xdrg_rpc_hdr *d_hdrs, uint64_t n, const uint64_t *d_reply_of, uint64_t ncalls,
                        uint32_t unanswered, xdrg_rpc_call_stat *d_stats, void *stream) {
  if (unanswered != XDRG_RPCS_PENDING && unanswered != XDRG_RPCS_NETWORK_ERROR) return XDRG_EINVAL;
  if (ncalls && (!d_reply_of || !d_stats || (n && !d_hdrs))) return XDRG_EINVAL;
  if (misaligned(d_hdrs, 15) || misaligned(d_reply_of, 7) || misaligned(d_stats, 7)) return XDRG_EALIGN;
  if (ncalls == 0) return XDRG_OK;
  const uint64_t nb = tiles_of(ncalls);
  if (nb > 0x7fffffffull) return XDRG_EUNSUPPORTED;
  k_st_call_stats<><<<uint32_t(nb), kTileThreads, 0, static_cast<hipStream_t>(stream)>>>(d_hdrs, n, d_reply_of, ncalls,
                                                                                     unanswered, d_stats);
  HIPCHK(hipGetLastError());
  return XDRG_OK;
}

size_t xdrg_rpc_pending_retire_workspace_size(uint64_t ncalls) { return retire_ws_bytes(ncalls); }

int xdrg_rpc_pending_retire(const xdrg_rpc_call *d_calls, uint64_t ncalls, const uint64_t *d_reply_of,
                            xdrg_rpc_call *d_kept, uint64_t *d_kept_pos, uint64_t *d_count, void *d_workspace,
                            size_t workspace_bytes, void *stream) {
  if (ncalls > 0x7fffffffffffull) return XDRG_EUNSUPPORTED;
  if (!d_count || (ncalls && (!d_calls || !d_reply_of || !d_kept))) return XDRG_EINVAL;
  if (ncalls && (d_kept == d_calls || overlap(d_kept, ncalls * 8, d_calls, ncalls * 8))) return XDRG_EINVAL;
  if (misaligned(d_calls, 7) || misaligned(d_reply_of, 7) || misaligned(d_kept, 7) || misaligned(d_kept_pos, 7) ||
      misaligned(d_count, 7) || misaligned(d_workspace, 7))
    return XDRG_EALIGN;
  return launch_retire(
      ncalls, d_count, d_workspace, workspace_bytes, stream,
      [&](uint32_t nb, hipStream_t s, unsigned long long *tiles) {
        k_st_count<><<<nb, kTileThreads, 0, s>>>(d_reply_of, ncalls, tiles);
      },
      [&](uint32_t nb, hipStream_t s, unsigned long long *tiles) {
        k_st_scatter<><<<nb, kTileThreads, 0, s>>>(d_calls, ncalls, d_reply_of, tiles, d_kept, d_kept_pos);
      });
}

}  // extern "C"
