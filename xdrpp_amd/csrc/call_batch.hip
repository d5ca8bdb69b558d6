// The asynchronous client's send half on gfx950: the launchers of
// call_batch_kernels.h.
//
//   xdrg_rpc_next_xids    rpc_sock::get_xid() (xdrpp/msgsock.h:118-122) n
//                         times, every one followed by send_call
//   xdrg_rpc_call_batch   xdr_to_msg(hdr, args...) of asynchronous_client_base::
//                         invoke (xdrpp/arpc.h:41-59) for every call of a
//                         batch, the procedures mixed, in call order
//   xdrg_rpc_pending_add  rpc_sock::calls_ after the send_calls
//                         (xdrpp/msgsock.cc:227-232)
//
// Every call validates its arguments on the host before the first HIP call,
// launches kernels only (no memset or memcpy nodes: xdrgpu.h "Graph
// capture") and keeps no state.  The sources travel by value as kernel
// arguments, each kernel with the fields it needs (the claim 40 bytes a
// source, the sizes 16, the emit 40: every table stays under the 4 KiB
// kernel-argument area).
#include <hip/hip_runtime.h>

#include "call_batch_kernels.h"
#include "host_common.h"

namespace {

using namespace xdrg;
using namespace xdrg::dev;
using namespace xdrg::host;

static_assert(sizeof(xdrg_rpc_arg_src) == 64, "xdrg_rpc_arg_src is 64 bytes");

}  // namespace

extern "C" {

int xdrg_rpc_next_xids(const xdrg_rpc_call *d_calls, uint64_t ncalls, uint32_t last_xid, uint64_t n,
                       uint32_t *d_xids, void *stream) {
  if (ncalls > 0xffffffffull || n > 0xffffffffull || ncalls + n > 0xffffffffull) return XDRG_EINVAL;
  if ((ncalls && !d_calls) || (n && !d_xids)) return XDRG_EINVAL;
  if (misaligned(d_calls, 7) || misaligned(d_xids, 3)) return XDRG_EALIGN;
  if (n == 0) return XDRG_OK;
  const uint64_t nb = (n + kPendingThreads - 1) / kPendingThreads;
  k_cb_next_xids<<<uint32_t(nb), kPendingThreads, 0, static_cast<hipStream_t>(stream)>>>(d_calls, ncalls, last_xid,
                                                                                       n, d_xids);
  HIPCHK(hipGetLastError());
  return XDRG_OK;
}

size_t xdrg_rpc_call_batch_workspace_size(uint64_t n) { return stream_ws_bytes(n); }

int xdrg_rpc_call_batch(const uint32_t *d_xids, uint64_t n, const xdrg_rpc_arg_src *srcs, uint32_t nsrcs,
                        void *d_out, uint64_t out_capacity, uint64_t *d_offsets, xdrg_rpc_call *d_sent,
                        uint64_t *d_counts, void *d_workspace, size_t workspace_bytes, xdrg_status *d_status,
                        void *stream) {
  if (!d_offsets || !d_status || (n && !d_xids) || (nsrcs && !srcs) || nsrcs > XDRG_RPC_MAX_ARG_SRCS)
    return XDRG_EINVAL;
  if (!valid_srcs(srcs, nsrcs)) return XDRG_EINVAL;
  if (!d_out && out_capacity) return XDRG_EINVAL;
  if (misaligned(d_xids, 3) || misaligned(d_offsets, 7) || misaligned(d_sent, 7) || misaligned(d_counts, 7) ||
      misaligned(d_workspace, 7) || misaligned(d_out, 3))
    return XDRG_EALIGN;
  if (misaligned_srcs(srcs, nsrcs)) return XDRG_EALIGN;
  if (n && (!d_workspace || workspace_bytes < stream_ws_bytes(n))) return XDRG_ESPACE;
  const uint64_t nb = tiles_of(n);
  if (nb > 0x7fffffffull) return XDRG_EUNSUPPORTED;

  src_claim_table C = {};
  src_count_table N = {};
  cb_size_table Z = {};
  cb_emit_table E = {};
  const uint64_t cblocks = build_src_tables(
      srcs, nsrcs, C, N, [&](uint32_t k, const xdrg_rpc_arg_src &S, const uint64_t *offs, uint32_t fixed) {
        Z.e[k] = cb_size_src{offs, fixed};
        E.e[k] = cb_emit_src{S.d_bytes, offs, fixed, S.res, S.prog, S.vers, S.proc, 0u};
      });
  if (cblocks > 0x7fffffffull) return XDRG_EUNSUPPORTED;

  hipStream_t s = static_cast<hipStream_t>(stream);
  auto *counts = reinterpret_cast<unsigned long long *>(d_counts);
  if (n == 0) {
    HIPCHK(static_cast<hipError_t>(fill32(d_offsets, 0u, 2, stream)));
    HIPCHK(static_cast<hipError_t>(fill32(&d_status->total_bytes, 0u, 2, stream)));
    if (counts) {
      k_src_count_entries<><<<1, 64, 0, s>>>(N, nsrcs, counts, counts + 1);
      HIPCHK(hipGetLastError());
    }
    return XDRG_OK;
  }
  auto *owner = static_cast<unsigned long long *>(d_workspace);
  auto *tiles = owner + ws_owner(n) / 8;
  auto *won = tiles + ws_tiles(n) / 8;
  k_owner_fill<><<<uint32_t(nb), kTileThreads, 0, s>>>(owner, n);
  HIPCHK(hipGetLastError());
  if (cblocks) {
    k_src_claim<<<uint32_t(cblocks), kTileThreads, 0, s>>>(n, C, nsrcs, cb_usable{}, owner);
    HIPCHK(hipGetLastError());
  }
  k_cb_sizes<<<uint32_t(nb), kTileThreads, 0, s>>>(n, owner, Z, tiles, won);
  HIPCHK(hipGetLastError());
  k_tile_scan<1, 2><<<1, kScanThreads, 0, s>>>(
      tiles, won, nb, stream_totals{N, nsrcs, n, d_offsets + n, d_status, counts, counts ? counts + 1 : nullptr});
  HIPCHK(hipGetLastError());
  k_cb_emit<<<uint32_t(nb), kTileThreads, 0, s>>>(d_xids, n, owner, E, static_cast<uint8_t *>(d_out), out_capacity,
                                                 d_offsets, d_sent, tiles,
                                                 reinterpret_cast<unsigned long long *>(&d_status->first_error));
  HIPCHK(hipGetLastError());
  return XDRG_OK;
}

int xdrg_rpc_pending_add(const xdrg_rpc_call *d_calls, uint64_t ncalls, const xdrg_rpc_call *d_new, uint64_t n,
                         xdrg_rpc_call *d_merged, uint64_t *d_old_pos, uint64_t *d_new_pos, void *stream) {
  if (ncalls > 0x7fffffffffffull || n > 0x7fffffffffffull) return XDRG_EUNSUPPORTED;
  const uint64_t total = ncalls + n;
  if ((ncalls && !d_calls) || (n && !d_new) || (total && !d_merged)) return XDRG_EINVAL;
  if (total && (d_merged == d_calls || d_merged == d_new || overlap(d_merged, total * 8, d_calls, ncalls * 8) ||
                overlap(d_merged, total * 8, d_new, n * 8)))
    return XDRG_EINVAL;
  if (misaligned(d_calls, 7) || misaligned(d_new, 7) || misaligned(d_merged, 7) || misaligned(d_old_pos, 7) ||
      misaligned(d_new_pos, 7))
    return XDRG_EALIGN;
  if (total == 0) return XDRG_OK;
  const uint64_t nb = (total + kPendingThreads - 1) / kPendingThreads;
  if (nb > 0x7fffffffull) return XDRG_EUNSUPPORTED;
  k_cb_pending_add<<<uint32_t(nb), kPendingThreads, 0, static_cast<hipStream_t>(stream)>>>(
      d_calls, ncalls, d_new, n, d_merged, d_old_pos, d_new_pos);
  HIPCHK(hipGetLastError());
  return XDRG_OK;
}

}  // extern "C"
