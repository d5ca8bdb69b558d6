// Host helpers of the launchers built on verify_kernels.h (verify.hip,
// replies.hip): the gather's launches and the geometry of a verify launch.
#pragma once
#include "host_common.h"
#include "verify_kernels.h"

namespace xdrg {
namespace host {

// ------------------------------------------------------------------ gather
// The launches of a gather whose arguments its caller has checked: count ->
// scan -> emit with the selector K (dev::k_gather_*, verify_kernels.h).
template <class SEL>
int launch_gather(const SEL &K, const void *d_stream, uint64_t len, const xdrg_rpc_hdr *d_hdrs, uint64_t n,
                  uint8_t *d_out, uint64_t capacity, uint64_t *d_offsets, uint64_t *d_index, uint64_t *d_count,
                  void *d_workspace, size_t workspace_bytes, xdrg_status *d_status, void *stream) {
  if (n == 0) {
    HIPCHK(static_cast<hipError_t>(fill32(d_offsets, 0u, 2, stream)));
    HIPCHK(static_cast<hipError_t>(fill32(d_count, 0u, 2, stream)));
    HIPCHK(static_cast<hipError_t>(fill32(&d_status->total_bytes, 0u, 2, stream)));
    return XDRG_OK;
  }
  if (!d_workspace || workspace_bytes < gather_ws_bytes(n)) return XDRG_ESPACE;
  const uint64_t nb = tiles_of(n);
  if (nb > 0x7fffffffull) return XDRG_EUNSUPPORTED;
  hipStream_t s = static_cast<hipStream_t>(stream);
  auto *tcnt = static_cast<unsigned long long *>(d_workspace);
  auto *tbytes = tcnt + ws_tiles(n) / 8;
  dev::k_gather_count<<<uint32_t(nb), dev::kTileThreads, 0, s>>>(d_hdrs, n, len, K, tcnt, tbytes);
  HIPCHK(hipGetLastError());
  dev::k_tile_scan<2, 2><<<1, dev::kScanThreads, 0, s>>>(tcnt, tbytes, nb,
                                                         dev::gather_totals{d_count, d_offsets, d_status});
  HIPCHK(hipGetLastError());
  dev::k_gather_emit<<<uint32_t(nb), dev::kTileThreads, 0, s>>>(
      static_cast<const uint8_t *>(d_stream), len, d_hdrs, n, K, d_out, capacity, d_offsets, d_index, tcnt, tbytes,
      reinterpret_cast<unsigned long long *>(&d_status->first_error));
  HIPCHK(hipGetLastError());
  return XDRG_OK;
}

// ------------------------------------------------------------------ verify
// The geometry of a verify launch (dev::k_verify, k_rpc_verify_args,
// k_rpc_verify_results): `sub` plans hold element subroutines (frames after
// the ops in LDS, smaller workgroups); the ops are staged in LDS when they fit
// the 48 KiB a workgroup may ask for without opting in to more.
struct verify_geom {
  uint32_t nt;
  uint64_t nb;
  size_t lds;
  bool lds_ops;
};
inline verify_geom verify_geometry(bool sub, size_t ops_bytes, uint64_t n) {
  const uint32_t nt = sub ? dev::kVerifySubThreads : dev::kVerifyThreads;
  const size_t frames = sub ? 4u * dev::verify_frame_words(nt) : 0u;
  const bool fit = ops_bytes + frames <= (48u << 10);
  return verify_geom{nt, (n + nt - 1) / nt, frames + (fit ? ops_bytes : 0u), fit};
}

}  // namespace host
}  // namespace xdrg
