// The asynchronous client over many connections on gfx950: the launchers of
// socks_kernels.h.  One table for every rpc_sock, sorted by (sock, xid):
//
//   xdrg_rpc_socks_next_xids       get_xid() (xdrpp/msgsock.h:118-122) with
//                                  every socket's own xid_ and calls_
//   xdrg_rpc_socks_pending_add     send_call's emplace (msgsock.cc:227-232)
//                                  into every socket's calls_
//   xdrg_rpc_socks_match_replies   recv_msg (msgsock.cc:202-232): a reply is
//                                  looked up in the calls_ of the socket it
//                                  arrived on
//   xdrg_rpc_socks_call_stats      rpc_call_stat(hdr) (rpc_msg.cc:69-90);
//                                  NETWORK_ERROR (arpc.h:60-61) for the calls
//                                  abort_all_calls (msgsock.cc:190-200) found
//                                  on a closed socket, and on no other
//   xdrg_rpc_socks_pending_retire  every calls_ after the erases and the aborts
//
// All validate on the host before the first HIP call, launch kernels only (no
// memset or memcpy nodes: xdrgpu.h "Graph capture") and keep no state.
#include <hip/hip_runtime.h>

#include "pending_host.h"
#include "socks_kernels.h"

namespace {

using namespace xdrg;
using namespace xdrg::dev;
using namespace xdrg::host;

}  // namespace

extern "C" {

int xdrg_rpc_socks_next_xids(const xdrg_rpc_call *d_calls, const uint32_t *d_sock, uint64_t ncalls,
                             const uint32_t *d_last, uint64_t nsocks, const uint32_t *d_call_sock, uint64_t n,
                             uint32_t *d_xids, uint32_t *d_last_out, void *stream) {
  if (ncalls > 0xffffffffull || n > 0xffffffffull || ncalls + n > 0xffffffffull || nsocks > 0xffffffffull)
    return XDRG_EINVAL;
  if ((ncalls && (!d_calls || !d_sock)) || (n && (!d_xids || !d_call_sock)) || (nsocks && !d_last))
    return XDRG_EINVAL;
  if (d_last_out && nsocks && (d_last_out == d_last || overlap(d_last_out, nsocks * 4, d_last, nsocks * 4)))
    return XDRG_EINVAL;
  if (misaligned(d_calls, 7) || misaligned(d_sock, 3) || misaligned(d_last, 3) || misaligned(d_call_sock, 3) ||
      misaligned(d_xids, 3) || misaligned(d_last_out, 3))
    return XDRG_EALIGN;
  const uint64_t lanes = n + (d_last_out ? nsocks : 0u);
  if (lanes == 0) return XDRG_OK;
  const uint64_t nb = (lanes + kPendingThreads - 1) / kPendingThreads;
  k_sk_next_xids<<<uint32_t(nb), kPendingThreads, 0, static_cast<hipStream_t>(stream)>>>(
      d_calls, d_sock, ncalls, d_last, nsocks, d_call_sock, n, d_xids, d_last_out);
  HIPCHK(hipGetLastError());
  return XDRG_OK;
}

int xdrg_rpc_socks_pending_add(const xdrg_rpc_call *d_calls, const uint32_t *d_sock, uint64_t ncalls,
                               const xdrg_rpc_call *d_new, const uint32_t *d_new_sock, uint64_t n,
                               xdrg_rpc_call *d_merged, uint32_t *d_merged_sock, uint64_t *d_old_pos,
                               uint64_t *d_new_pos, void *stream) {
  if (ncalls > 0x7fffffffffffull || n > 0x7fffffffffffull) return XDRG_EUNSUPPORTED;
  const uint64_t total = ncalls + n;
  if ((ncalls && (!d_calls || !d_sock)) || (n && (!d_new || !d_new_sock)) || (total && (!d_merged || !d_merged_sock)))
    return XDRG_EINVAL;
  if (total) {
    if (d_merged == d_calls || d_merged == d_new || overlap(d_merged, total * 8, d_calls, ncalls * 8) ||
        overlap(d_merged, total * 8, d_new, n * 8))
      return XDRG_EINVAL;
    if (d_merged_sock == d_sock || d_merged_sock == d_new_sock ||
        overlap(d_merged_sock, total * 4, d_sock, ncalls * 4) || overlap(d_merged_sock, total * 4, d_new_sock, n * 4))
      return XDRG_EINVAL;
  }
  if (misaligned(d_calls, 7) || misaligned(d_new, 7) || misaligned(d_merged, 7) || misaligned(d_old_pos, 7) ||
      misaligned(d_new_pos, 7) || misaligned(d_sock, 3) || misaligned(d_new_sock, 3) || misaligned(d_merged_sock, 3))
    return XDRG_EALIGN;
  if (total == 0) return XDRG_OK;
  const uint64_t nb = (total + kPendingThreads - 1) / kPendingThreads;
  if (nb > 0x7fffffffull) return XDRG_EUNSUPPORTED;
  k_sk_pending_add<<<uint32_t(nb), kPendingThreads, 0, static_cast<hipStream_t>(stream)>>>(
      d_calls, d_sock, ncalls, d_new, d_new_sock, n, d_merged, d_merged_sock, d_old_pos, d_new_pos);
  HIPCHK(hipGetLastError());
  return XDRG_OK;
}

int xdrg_rpc_socks_match_replies(const void *d_stream, uint64_t len, const uint64_t *d_offsets, uint64_t n,
                                 const uint32_t *d_msg_row, const uint32_t *d_row_sock, uint64_t nrows,
                                 const xdrg_rpc_call *d_calls, const uint32_t *d_sock, uint64_t ncalls,
                                 xdrg_rpc_hdr *d_hdrs, uint64_t *d_call, uint64_t *d_reply_of, void *stream) {
  if (n && (!d_offsets || !d_hdrs || !d_call || !d_msg_row || (!d_stream && len))) return XDRG_EINVAL;
  if (ncalls && (!d_calls || !d_sock || !d_reply_of)) return XDRG_EINVAL;
  if (misaligned(d_stream, 3) || misaligned(d_offsets, 7) || misaligned(d_calls, 7) || misaligned(d_hdrs, 15) ||
      misaligned(d_call, 7) || misaligned(d_reply_of, 7) || misaligned(d_msg_row, 3) || misaligned(d_row_sock, 3) ||
      misaligned(d_sock, 3))
    return XDRG_EALIGN;
  return launch_match(n, ncalls, d_hdrs, d_call, d_reply_of, stream,
                      [&](uint32_t nb, hipStream_t s, unsigned long long *call, unsigned long long *reply_of) {
                        k_sk_claim<<<nb, kPendingThreads, 0, s>>>(static_cast<const uint8_t *>(d_stream), len,
                                                                  d_offsets, n, d_msg_row, d_row_sock, nrows, d_calls,
                                                                  d_sock, ncalls, call, reply_of);
                      });
}

int xdrg_rpc_socks_call_stats(const xdrg_rpc_hdr *d_hdrs, uint64_t n, const uint64_t *d_reply_of,
                              const uint32_t *d_sock, uint64_t ncalls, const uint32_t *d_closed, uint64_t nsocks,
                              xdrg_rpc_call_stat *d_stats, void *stream) {
  if (ncalls && (!d_reply_of || !d_sock || !d_stats || (n && !d_hdrs) || (nsocks && !d_closed))) return XDRG_EINVAL;
  if (misaligned(d_hdrs, 15) || misaligned(d_reply_of, 7) || misaligned(d_stats, 7) || misaligned(d_sock, 3) ||
      misaligned(d_closed, 3))
    return XDRG_EALIGN;
  if (ncalls == 0) return XDRG_OK;
  const uint64_t nb = tiles_of(ncalls);
  if (nb > 0x7fffffffull) return XDRG_EUNSUPPORTED;
  k_sk_call_stats<<<uint32_t(nb), kTileThreads, 0, static_cast<hipStream_t>(stream)>>>(
      d_hdrs, n, d_reply_of, d_sock, ncalls, d_closed, nsocks, d_stats);
  HIPCHK(hipGetLastError());
  return XDRG_OK;
}

size_t xdrg_rpc_socks_pending_retire_workspace_size(uint64_t ncalls) { return retire_ws_bytes(ncalls); }

int xdrg_rpc_socks_pending_retire(const xdrg_rpc_call *d_calls, const uint32_t *d_sock, uint64_t ncalls,
                                  const uint64_t *d_reply_of, const uint32_t *d_closed, uint64_t nsocks,
                                  xdrg_rpc_call *d_kept, uint32_t *d_kept_sock, uint64_t *d_kept_pos,
                                  uint64_t *d_count, void *d_workspace, size_t workspace_bytes, void *stream) {
  if (ncalls > 0x7fffffffffffull) return XDRG_EUNSUPPORTED;
  if (!d_count ||
      (ncalls && (!d_calls || !d_sock || !d_reply_of || !d_kept || !d_kept_sock || (nsocks && !d_closed))))
    return XDRG_EINVAL;
  if (ncalls && (d_kept == d_calls || overlap(d_kept, ncalls * 8, d_calls, ncalls * 8) || d_kept_sock == d_sock ||
                 overlap(d_kept_sock, ncalls * 4, d_sock, ncalls * 4)))
    return XDRG_EINVAL;
  if (misaligned(d_calls, 7) || misaligned(d_reply_of, 7) || misaligned(d_kept, 7) || misaligned(d_kept_pos, 7) ||
      misaligned(d_count, 7) || misaligned(d_workspace, 7) || misaligned(d_sock, 3) || misaligned(d_closed, 3) ||
      misaligned(d_kept_sock, 3))
    return XDRG_EALIGN;
  return launch_retire(
      ncalls, d_count, d_workspace, workspace_bytes, stream,
      [&](uint32_t nb, hipStream_t s, unsigned long long *tiles) {
        k_sk_count<<<nb, kTileThreads, 0, s>>>(d_reply_of, d_sock, ncalls, d_closed, nsocks, tiles);
      },
      [&](uint32_t nb, hipStream_t s, unsigned long long *tiles) {
        k_sk_scatter<<<nb, kTileThreads, 0, s>>>(d_calls, d_sock, ncalls, d_reply_of, d_closed, nsocks, tiles, d_kept,
                                                 d_kept_sock, d_kept_pos);
      });
}

}  // extern "C"
