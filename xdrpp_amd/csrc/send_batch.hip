// The send batch on gfx950: the launcher of send_batch_kernels.h.
//
//   xdrg_rpc_send_batch  msg_sock::putmsg for many streams and connections at
//                        once (xdrpp/msgsock.cc:121-134): every connection's
//                        messages contiguous and in putmsg order in one
//                        stream, a queue record per connection (wqueue_,
//                        wsize_), a closed connection's messages dropped
//                        (wfail_, :124-127)
//
// Validates on the host before the first HIP call, launches kernels only (no
// memset or memcpy node: xdrgpu.h "Graph capture") and keeps no state.  The
// launch sequence depends on the host arguments alone: whether the sort
// passes have anything to do is decided on the device (sb_ctl::inorder).
#include <hip/hip_runtime.h>

#include "host_common.h"
#include "send_batch_kernels.h"

namespace {

using namespace xdrg;
using namespace xdrg::dev;
using namespace xdrg::host;

// 8-bit digits that hold every key, the sentinel nconns included
uint32_t sb_passes(uint64_t nconns) {
  uint32_t bits = 0;
  while (bits < 32 && (nconns >> bits)) ++bits;
  return (bits + 7) / 8;
}
uint64_t sb_sort_tiles(uint64_t entries) { return (entries + kSbSortTile - 1) / kSbSortTile; }

// the keyed items, the other side of the passes, the (digit, tile) counts,
// two tile columns (the keys' counts, then the sizes'), sb_ctl
size_t sb_items_bytes(uint64_t entries) { return align256(entries * 8); }
size_t sb_passed_at(uint64_t entries) { return sb_items_bytes(entries); }
size_t sb_hist_at(uint64_t entries, uint64_t nconns) {
  return sb_passed_at(entries) + (sb_passes(nconns) ? sb_items_bytes(entries) : 0);
}
size_t sb_tiles_at(uint64_t entries, uint64_t nconns) {
  return sb_hist_at(entries, nconns) + (sb_passes(nconns) ? align256(256 * sb_sort_tiles(entries) * 4) : 0);
}
size_t sb_ctl_at(uint64_t entries, uint64_t nconns) { return sb_tiles_at(entries, nconns) + 2 * ws_tiles(entries); }
size_t sb_ws_bytes(uint64_t entries, uint64_t nconns) { return sb_ctl_at(entries, nconns) + 256; }

}  // namespace

extern "C" {

size_t xdrg_rpc_send_batch_workspace_size(uint64_t entries, uint64_t nconns) {
  return sb_ws_bytes(entries, nconns > 0x7fffffffull ? 0x7fffffffull : nconns);
}

int xdrg_rpc_send_batch(const xdrg_rpc_send_src *srcs, uint32_t nsrcs, uint64_t nconns, const uint32_t *d_closed,
                        void *d_out, uint64_t out_capacity, uint64_t *d_offsets, uint64_t *d_count,
                        uint32_t *d_conn_of, uint64_t *d_from, int64_t *d_pos, xdrg_rpc_wqueue *d_queues,
                        uint64_t *d_counts, void *d_workspace, size_t workspace_bytes, xdrg_status *d_status,
                        void *stream) {
  if (!d_offsets || !d_count || !d_status || (nsrcs && !srcs) || nsrcs > XDRG_RPC_MAX_SEND_SRCS) return XDRG_EINVAL;
  if ((out_capacity && !d_out) || (nconns && !d_queues)) return XDRG_EINVAL;
  uint64_t entries = 0;
  for (uint32_t k = 0; k < nsrcs; ++k) {
    const xdrg_rpc_send_src &S = srcs[k];
    if ((S.count_cap && !S.d_offsets) || (S.bytes_len && !S.d_bytes)) return XDRG_EINVAL;
    if (overlap(d_out, out_capacity, S.d_bytes, S.bytes_len)) return XDRG_EINVAL;
    entries += S.count_cap;
  }
  if (entries && (!d_conn_of || !d_from)) return XDRG_EINVAL;
  for (uint32_t k = 0; k < nsrcs; ++k)
    if (misaligned(srcs[k].d_bytes, 3) || misaligned(srcs[k].d_offsets, 7) || misaligned(srcs[k].d_conn, 3) ||
        misaligned(srcs[k].d_count, 7))
      return XDRG_EALIGN;
  if (misaligned(d_out, 3) || misaligned(d_closed, 3) || misaligned(d_conn_of, 3) || misaligned(d_offsets, 7) ||
      misaligned(d_count, 7) || misaligned(d_from, 7) || misaligned(d_pos, 7) || misaligned(d_queues, 7) ||
      misaligned(d_counts, 7) || misaligned(d_status, 7) || misaligned(d_workspace, 7))
    return XDRG_EALIGN;
  if (entries > 0xffffffffull || nconns > 0x7fffffffull) return XDRG_EUNSUPPORTED;
  if (!d_workspace || workspace_bytes < sb_ws_bytes(entries, nconns)) return XDRG_ESPACE;

  sb_table T = {};
  src_count_table N = {};
  uint64_t at = 0;
  for (uint32_t k = 0; k < nsrcs; ++k) {
    const xdrg_rpc_send_src &S = srcs[k];
    T.e[k] = sb_src{S.d_bytes, S.d_offsets, S.d_conn, S.d_count, S.bytes_len, S.count_cap, S.conn};
    T.base[k] = uint32_t(at);
    N.count[k] = S.d_count;
    N.cap[k] = S.count_cap;
    at += S.count_cap;
  }
  for (uint32_t k = nsrcs; k <= kMaxSrcs; ++k) T.base[k] = uint32_t(at);

  hipStream_t s = static_cast<hipStream_t>(stream);
  const uint32_t passes = sb_passes(nconns);
  const uint64_t nb = tiles_of(entries), nt = sb_sort_tiles(entries);
  auto *ws = static_cast<uint8_t *>(d_workspace);
  auto *keyed = reinterpret_cast<unsigned long long *>(ws);
  auto *other = reinterpret_cast<unsigned long long *>(ws + sb_passed_at(entries));
  auto *hist = reinterpret_cast<uint32_t *>(ws + sb_hist_at(entries, nconns));
  auto *tile_a = reinterpret_cast<unsigned long long *>(ws + sb_tiles_at(entries, nconns));
  auto *tile_b = reinterpret_cast<unsigned long long *>(ws + sb_tiles_at(entries, nconns) + ws_tiles(entries));
  auto *ctl = reinterpret_cast<sb_ctl *>(ws + sb_ctl_at(entries, nconns));
  auto *pos = reinterpret_cast<long long *>(d_pos);

  if (nb) {
    k_sb_keys<<<uint32_t(nb), kTileThreads, 0, s>>>(T, nsrcs, entries, nconns, d_closed, keyed, pos, tile_a, tile_b);
    HIPCHK(hipGetLastError());
  }
  k_tile_scan<1, 2><<<1, kScanThreads, 0, s>>>(tile_a, tile_b, nb, sb_key_totals{N, nsrcs, d_counts, ctl});
  HIPCHK(hipGetLastError());
  for (uint32_t p = 0; nb && p < passes; ++p) {
    const unsigned long long *in = (p & 1u) ? other : keyed;
    unsigned long long *out = (p & 1u) ? keyed : other;
    k_sb_hist<<<uint32_t(nt), kTileThreads, 0, s>>>(ctl, in, entries, 8u * p, nt, hist);
    HIPCHK(hipGetLastError());
    k_sb_pass_scan<<<1, kScanThreads, 0, s>>>(ctl, hist, 256 * nt);
    HIPCHK(hipGetLastError());
    k_sb_scatter<<<uint32_t(nt), kTileThreads, 0, s>>>(ctl, in, entries, 8u * p, nt, hist, out);
    HIPCHK(hipGetLastError());
  }
  const sb_sorted sorted{ctl, keyed, (passes & 1u) ? other : keyed};
  if (nb) {
    k_sb_sizes<<<uint32_t(nb), kTileThreads, 0, s>>>(sorted, entries, nconns, T, nsrcs, d_conn_of, d_from, pos, tile_a,
                                                     tile_b);
    HIPCHK(hipGetLastError());
  }
  k_tile_scan<2, 2><<<1, kScanThreads, 0, s>>>(tile_a, tile_b, nb, gather_totals{d_count, d_offsets, d_status});
  HIPCHK(hipGetLastError());
  if (nb) {
    k_sb_emit<16><<<uint32_t(nb), kTileThreads, 0, s>>>(sorted, entries, nconns, T, nsrcs,
                                                        static_cast<uint8_t *>(d_out), out_capacity, d_offsets, tile_b,
                                                        reinterpret_cast<unsigned long long *>(&d_status->first_error));
    HIPCHK(hipGetLastError());
  }
  if (nconns) {
    k_sb_queues<<<uint32_t(tiles_of(nconns)), kTileThreads, 0, s>>>(sorted, entries, nconns, d_offsets, d_queues);
    HIPCHK(hipGetLastError());
  }
  return XDRG_OK;
}

}  // extern "C"
