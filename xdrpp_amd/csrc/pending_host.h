// Host helpers of the launchers built on pending_kernels.h (replies.hip,
// settle.hip, socks.hip): the launches of a match and of a retire whose
// arguments the caller has checked.
#pragma once
#include "host_common.h"
#include "pending_kernels.h"

namespace xdrg {
namespace host {

// ------------------------------------------------------------------- match
// fill -> claim -> resolve.  claim(nb, s, call, reply_of) launches the stage's
// claim kernel, nb workgroups of kPendingThreads.
template <class CLAIM>
int launch_match(uint64_t n, uint64_t ncalls, xdrg_rpc_hdr *d_hdrs, uint64_t *d_call, uint64_t *d_reply_of,
                 void *stream, CLAIM &&claim) {
  if (n == 0 && ncalls == 0) return XDRG_OK;
  const uint64_t nb = (n + dev::kPendingThreads - 1) / dev::kPendingThreads;
  if (nb > 0x7fffffffull || ncalls > 0x7fffffffffffull) return XDRG_EUNSUPPORTED;
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (ncalls) HIPCHK(static_cast<hipError_t>(fill32(d_reply_of, 0xffffffffu, 2 * ncalls, stream)));
  if (n == 0) return XDRG_OK;
  auto *call = reinterpret_cast<unsigned long long *>(d_call);
  auto *reply_of = reinterpret_cast<unsigned long long *>(d_reply_of);
  claim(uint32_t(nb), s, call, reply_of);
  HIPCHK(hipGetLastError());
  dev::k_pending_resolve<><<<uint32_t(nb), dev::kPendingThreads, 0, s>>>(d_hdrs, n, call, reply_of);
  HIPCHK(hipGetLastError());
  return XDRG_OK;
}

// ------------------------------------------------------------------ retire
// the kept entries of every tile, one word each
inline size_t retire_ws_bytes(uint64_t ncalls) { return align256(tiles_of(ncalls) * 8); }

// count -> scan -> scatter.  count(nb, s, tiles) and scatter(nb, s, tiles)
// launch the stage's two kernels, nb workgroups of kTileThreads.
template <class COUNT, class SCATTER>
int launch_retire(uint64_t ncalls, uint64_t *d_count, void *d_workspace, size_t workspace_bytes, void *stream,
                  COUNT &&count, SCATTER &&scatter) {
  if (ncalls && (!d_workspace || workspace_bytes < retire_ws_bytes(ncalls))) return XDRG_ESPACE;
  const uint64_t nb = tiles_of(ncalls);
  if (nb > 0x7fffffffull) return XDRG_EUNSUPPORTED;
  hipStream_t s = static_cast<hipStream_t>(stream);
  auto *tiles = static_cast<unsigned long long *>(d_workspace);
  if (nb) {
    count(uint32_t(nb), s, tiles);
    HIPCHK(hipGetLastError());
  }
  // nb == 0: the count alone
  dev::k_tile_scan<1, 1><<<1, dev::kScanThreads, 0, s>>>(tiles, nullptr, nb, dev::count_total{d_count});
  HIPCHK(hipGetLastError());
  if (nb) {
    scatter(uint32_t(nb), s, tiles);
    HIPCHK(hipGetLastError());
  }
  return XDRG_OK;
}

}  // namespace host
}  // namespace xdrg
