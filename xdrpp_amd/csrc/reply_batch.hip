// The server's reply stream on gfx950: the launcher of reply_batch_kernels.h.
//
//   xdrg_rpc_reply_batch   srpc_service::dispatch's reply (xdrpp/srpc.h:130-153)
//                          for every message of a dispatched batch, success
//                          and error replies in the order srpc_server::run
//                          writes them (xdrpp/srpc.cc:83-88)
//
// The call validates its arguments on the host before the first HIP call,
// launches kernels only (no memset or memcpy nodes: xdrgpu.h "Graph
// capture") and keeps no state.  The sources travel by value as kernel
// arguments, each kernel with the fields it needs (the claim 40 bytes a
// source, the sizes and the emit 24: both tables stay under the 4 KiB
// kernel-argument area).
#include <hip/hip_runtime.h>

#include <cstdlib>

#include "host_common.h"
#include "reply_batch_kernels.h"

namespace {

using namespace xdrg;
using namespace xdrg::dev;
using namespace xdrg::host;

// Bytes a lane of the emit writes per step: 16 (aligned chunks), or 4 with
// XDRG_REPLY_BATCH_COPY=4 in the environment (tools/gpu/time_reply_batch.py
// measures both).
int copy_width() {
  const char *v = std::getenv("XDRG_REPLY_BATCH_COPY");
  return v && v[0] == '4' && !v[1] ? 4 : 16;
}

}  // namespace

extern "C" {

size_t xdrg_rpc_reply_batch_workspace_size(uint64_t n) { return stream_ws_bytes(n); }

int xdrg_rpc_reply_batch(const xdrg_rpc_hdr *d_hdrs, uint64_t n, const xdrg_rpc_result_src *srcs, uint32_t nsrcs,
                         void *d_out, uint64_t out_capacity, uint64_t *d_offsets, uint64_t *d_unused,
                         void *d_workspace, size_t workspace_bytes, xdrg_status *d_status, void *stream) {
  if (!d_offsets || !d_status || (n && !d_hdrs) || (nsrcs && !srcs) || nsrcs > XDRG_RPC_MAX_RESULT_SRCS)
    return XDRG_EINVAL;
  if (!valid_srcs(srcs, nsrcs)) return XDRG_EINVAL;
  if (!d_out && out_capacity) return XDRG_EINVAL;
  if (misaligned(d_hdrs, 15) || misaligned(d_offsets, 7) || misaligned(d_unused, 7) || misaligned(d_workspace, 7) ||
      misaligned(d_out, 3))
    return XDRG_EALIGN;
  if (misaligned_srcs(srcs, nsrcs)) return XDRG_EALIGN;
  if (n && (!d_workspace || workspace_bytes < stream_ws_bytes(n))) return XDRG_ESPACE;
  const uint64_t nb = tiles_of(n);
  if (nb > 0x7fffffffull) return XDRG_EUNSUPPORTED;

  src_claim_table C = {};
  src_count_table N = {};
  rb_span_table P = {};
  const uint64_t cblocks = build_src_tables(
      srcs, nsrcs, C, N, [&](uint32_t k, const xdrg_rpc_result_src &S, const uint64_t *offs, uint32_t fixed) {
        P.e[k] = rb_span_src{S.d_bytes, offs, fixed};
      });
  if (cblocks > 0x7fffffffull) return XDRG_EUNSUPPORTED;

  hipStream_t s = static_cast<hipStream_t>(stream);
  auto *unused = reinterpret_cast<unsigned long long *>(d_unused);
  if (n == 0) {
    HIPCHK(static_cast<hipError_t>(fill32(d_offsets, 0u, 2, stream)));
    HIPCHK(static_cast<hipError_t>(fill32(&d_status->total_bytes, 0u, 2, stream)));
    if (unused) {
      k_src_count_entries<><<<1, 64, 0, s>>>(N, nsrcs, nullptr, unused);
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
    k_src_claim<<<uint32_t(cblocks), kTileThreads, 0, s>>>(n, C, nsrcs, rb_usable{d_hdrs}, owner);
    HIPCHK(hipGetLastError());
  }
  k_rb_sizes<<<uint32_t(nb), kTileThreads, 0, s>>>(d_hdrs, n, owner, P, tiles, won);
  HIPCHK(hipGetLastError());
  k_tile_scan<1, 2><<<1, kScanThreads, 0, s>>>(
      tiles, won, nb, stream_totals{N, nsrcs, n, d_offsets + n, d_status, nullptr, unused});
  HIPCHK(hipGetLastError());
  auto *err = reinterpret_cast<unsigned long long *>(&d_status->first_error);
  uint8_t *out = static_cast<uint8_t *>(d_out);
  if (copy_width() == 4)
    k_rb_emit<4><<<uint32_t(nb), kTileThreads, 0, s>>>(d_hdrs, n, owner, P, out, out_capacity, d_offsets, tiles, err);
  else
    k_rb_emit<16><<<uint32_t(nb), kTileThreads, 0, s>>>(d_hdrs, n, owner, P, out, out_capacity, d_offsets, tiles, err);
  HIPCHK(hipGetLastError());
  return XDRG_OK;
}

}  // extern "C"
