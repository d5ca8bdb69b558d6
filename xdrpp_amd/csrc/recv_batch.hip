// The receive batch on gfx950: the launcher of recv_batch_kernels.h.
//
//   xdrg_rpc_recv_batch  msg_sock::input for many connections at once
//                        (xdrpp/msgsock.cc:38-119): every whole message of
//                        every connection in one stream with its index, the
//                        partial tail left to the next read (rdpos_, rdmsg_),
//                        a framing error closing its own connection only; with
//                        XDRG_RECV_RPC_SOCK rpc_sock::recv_msg's test
//                        (msgsock.cc:202-225)
//
// Validates on the host before the first HIP call, launches kernels only (no
// memset or memcpy node: xdrgpu.h "Graph capture") and keeps no state.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "host_common.h"
#include "recv_batch_kernels.h"

namespace {

using namespace xdrg;
using namespace xdrg::dev;
using namespace xdrg::host;

// tile messages, tile bytes, every connection's base in the stream, the list
// of the wave pass, rb_ctl
size_t rb_cbase_at(uint64_t nconns) { return 2 * ws_tiles(nconns); }
size_t rb_list_at(uint64_t nconns) { return rb_cbase_at(nconns) + align256(nconns * 8); }
size_t rb_ctl_at(uint64_t nconns) { return rb_list_at(nconns) + align256(nconns * 4); }
size_t rb_ws_bytes(uint64_t nconns) { return rb_ctl_at(nconns) + 256; }

}  // namespace

extern "C" {

// buf_len: the walk logs nothing per word, so the buffer's length adds nothing.
size_t xdrg_rpc_recv_batch_workspace_size(uint64_t nconns, uint64_t /*buf_len*/) { return rb_ws_bytes(nconns); }

int xdrg_rpc_recv_batch(const void *d_buf, uint64_t buf_len, const xdrg_rpc_conn_in *d_segs, uint64_t nconns,
                        uint32_t max_msg_len, uint32_t flags, void *d_out, uint64_t out_capacity, uint64_t *d_offsets,
                        uint64_t max_msgs, uint64_t *d_count, uint32_t *d_conn_of, uint8_t *d_kind,
                        xdrg_rpc_conn *d_conns, void *d_workspace, size_t workspace_bytes, xdrg_status *d_status,
                        void *stream) {
  if (flags & ~XDRG_RECV_RPC_SOCK) return XDRG_EINVAL;
  if (!d_offsets || !d_count || !d_status) return XDRG_EINVAL;
  if (nconns && (!d_segs || !d_conns)) return XDRG_EINVAL;
  if ((buf_len && !d_buf) || (out_capacity && !d_out) || (max_msgs && !d_conn_of)) return XDRG_EINVAL;
  if ((flags & XDRG_RECV_RPC_SOCK) && max_msgs && !d_kind) return XDRG_EINVAL;
  if (overlap(d_out, out_capacity, d_buf, buf_len)) return XDRG_EINVAL;
  if (misaligned(d_buf, 3) || misaligned(d_out, 3) || misaligned(d_segs, 7) || misaligned(d_offsets, 7) ||
      misaligned(d_count, 7) || misaligned(d_conn_of, 3) || misaligned(d_conns, 7) || misaligned(d_status, 7) ||
      misaligned(d_workspace, 7))
    return XDRG_EALIGN;
  if (nconns > 0x7fffffffull || max_msgs > 0xffffffffffull) return XDRG_EUNSUPPORTED;  // d_conn_of; the status key
  if (nconns && (!d_workspace || workspace_bytes < rb_ws_bytes(nconns))) return XDRG_ESPACE;

  hipStream_t s = static_cast<hipStream_t>(stream);
  const uint64_t nb = tiles_of(nconns);
  auto *ws = static_cast<uint8_t *>(d_workspace);
  auto *tile_msgs = reinterpret_cast<unsigned long long *>(ws);
  auto *tile_bytes = reinterpret_cast<unsigned long long *>(ws + (nconns ? ws_tiles(nconns) : 0));
  const rb_totals totals{d_count, d_offsets, max_msgs, d_status};
  if (!nb) {  // the totals alone
    k_tile_scan<2, 2><<<1, kScanThreads, 0, s>>>(tile_msgs, tile_bytes, 0, totals);
    HIPCHK(hipGetLastError());
    return XDRG_OK;
  }
  auto *cbase = reinterpret_cast<unsigned long long *>(ws + rb_cbase_at(nconns));
  auto *list = reinterpret_cast<uint32_t *>(ws + rb_list_at(nconns));
  auto *ctl = reinterpret_cast<rb_ctl *>(ws + rb_ctl_at(nconns));
  const rb_args A{static_cast<const uint8_t *>(d_buf), buf_len, d_segs, nconns, max_msg_len,
                  flags & XDRG_RECV_RPC_SOCK};
  const rb_outs O{d_offsets, max_msgs, out_capacity, d_conn_of, (flags & XDRG_RECV_RPC_SOCK) ? d_kind : nullptr,
                  reinterpret_cast<unsigned long long *>(&d_status->first_error), ctl};
  const uint32_t wgrid = uint32_t(std::min<uint64_t>(nconns, kRbWaveGrid));

  HIPCHK(static_cast<hipError_t>(fill32(&ctl->listed, 0u, 2, stream)));
  HIPCHK(static_cast<hipError_t>(fill32(&ctl->fit, 0xffffffffu, 2, stream)));
  k_rb_count<<<uint32_t(nb), kTileThreads, 0, s>>>(A, d_conns, tile_msgs, tile_bytes, list, ctl);
  HIPCHK(hipGetLastError());
  k_rb_count_wave<<<wgrid, 64, 0, s>>>(A, d_conns, tile_msgs, tile_bytes, list, ctl);
  HIPCHK(hipGetLastError());
  k_tile_scan<2, 2><<<1, kScanThreads, 0, s>>>(tile_msgs, tile_bytes, nb, totals);
  HIPCHK(hipGetLastError());
  k_rb_emit<<<uint32_t(nb), kTileThreads, 0, s>>>(A, d_conns, tile_msgs, tile_bytes, cbase, O);
  HIPCHK(hipGetLastError());
  k_rb_emit_wave<<<wgrid, 64, 0, s>>>(A, d_conns, cbase, list, O);
  HIPCHK(hipGetLastError());
  const uint64_t most = std::min<uint64_t>(out_capacity, buf_len);  // what disjoint segments can deliver
  if (most) {
    const uint32_t cgrid = uint32_t(std::min<uint64_t>(kRbCopyGrid, (most / 16 + 2 + 255) / 256));
    k_rb_copy<<<cgrid, 256, 0, s>>>(A, d_conns, cbase, ctl, static_cast<uint8_t *>(d_out), out_capacity);
    HIPCHK(hipGetLastError());
  }
  return XDRG_OK;
}

}  // extern "C"
