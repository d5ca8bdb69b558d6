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

#include "plan.h"
#include "reply_batch_kernels.h"

namespace {

using namespace xdrg;
using namespace xdrg::dev;

#define HIPCHK(x)                                                             \
  do {                                                                        \
    hipError_t e_ = (x);                                                      \
    if (e_ != hipSuccess) return xdrg::record_hip_error(int(e_), #x);         \
  } while (0)

bool misaligned(const void *p, uintptr_t mask) { return reinterpret_cast<uintptr_t>(p) & mask; }

size_t align256(size_t v) { return (v + 255) / 256 * 256; }
// owner words (n), then per 256-message tile the reply bytes and the winners (nb + 1 each)
size_t rb_ws_owner(uint64_t n) { return align256(n * 8); }
size_t rb_ws_tiles(uint64_t n) { return align256(((n + kRbThreads - 1) / kRbThreads + 1) * 8); }
size_t rb_ws_bytes(uint64_t n) { return rb_ws_owner(n) + 2 * rb_ws_tiles(n); }

// Bytes a lane of the emit writes per step: 16 (aligned chunks), or 4 with
// XDRG_REPLY_BATCH_COPY=4 in the environment (tools/gpu/time_reply_batch.py
// measures both).
int copy_width() {
  const char *v = std::getenv("XDRG_REPLY_BATCH_COPY");
  return v && v[0] == '4' && !v[1] ? 4 : 16;
}

}  // namespace

extern "C" {

size_t xdrg_rpc_reply_batch_workspace_size(uint64_t n) { return rb_ws_bytes(n); }

int xdrg_rpc_reply_batch(const xdrg_rpc_hdr *d_hdrs, uint64_t n, const xdrg_rpc_result_src *srcs, uint32_t nsrcs,
                         void *d_out, uint64_t out_capacity, uint64_t *d_offsets, uint64_t *d_unused,
                         void *d_workspace, size_t workspace_bytes, xdrg_status *d_status, void *stream) {
  if (!d_offsets || !d_status || (n && !d_hdrs) || (nsrcs && !srcs) || nsrcs > XDRG_RPC_MAX_RESULT_SRCS)
    return XDRG_EINVAL;
  for (uint32_t k = 0; k < nsrcs; ++k) {
    const xdrg_rpc_result_src &S = srcs[k];
    if (S.count_cap && !S.d_index) return XDRG_EINVAL;
    if (!S.d_bytes && S.fixed_size) return XDRG_EINVAL;
    if (S.d_bytes && !S.d_offsets && (!S.fixed_size || (S.fixed_size & 3u))) return XDRG_EINVAL;
  }
  if (!d_out && out_capacity) return XDRG_EINVAL;
  if (misaligned(d_hdrs, 15) || misaligned(d_offsets, 7) || misaligned(d_unused, 7) || misaligned(d_workspace, 7) ||
      misaligned(d_out, 3))
    return XDRG_EALIGN;
  for (uint32_t k = 0; k < nsrcs; ++k)
    if (misaligned(srcs[k].d_bytes, 3) || misaligned(srcs[k].d_offsets, 7) || misaligned(srcs[k].d_index, 7) ||
        misaligned(srcs[k].d_count, 7))
      return XDRG_EALIGN;
  if (n && (!d_workspace || workspace_bytes < rb_ws_bytes(n))) return XDRG_ESPACE;
  const uint64_t nb = (n + kRbThreads - 1) / kRbThreads;
  if (nb > 0x7fffffffull) return XDRG_EUNSUPPORTED;

  rb_claim_table C = {};
  rb_span_table P = {};
  rb_count_table N = {};
  uint64_t cblocks = 0;
  for (uint32_t k = 0; k < nsrcs; ++k) {
    const xdrg_rpc_result_src &S = srcs[k];
    const bool has = S.d_bytes != nullptr;  // a void source: every span is [0, 0)
    C.e[k] = rb_claim_src{S.d_index, S.d_count, has ? S.d_offsets : nullptr, S.bytes_len, S.count_cap,
                          has ? S.fixed_size : 0u};
    P.e[k] = rb_span_src{S.d_bytes, has ? S.d_offsets : nullptr, has ? S.fixed_size : 0u};
    N.count[k] = S.d_count;
    N.cap[k] = S.count_cap;
    C.blk[k] = uint32_t(cblocks);
    cblocks += (uint64_t(S.count_cap) + kRbThreads - 1) / kRbThreads;
  }
  if (cblocks > 0x7fffffffull) return XDRG_EUNSUPPORTED;
  for (uint32_t k = nsrcs; k <= XDRG_RPC_MAX_RESULT_SRCS; ++k) C.blk[k] = uint32_t(cblocks);

  hipStream_t s = static_cast<hipStream_t>(stream);
  auto *unused = reinterpret_cast<unsigned long long *>(d_unused);
  if (n == 0) {
    HIPCHK(static_cast<hipError_t>(fill32(d_offsets, 0u, 2, stream)));
    HIPCHK(static_cast<hipError_t>(fill32(&d_status->total_bytes, 0u, 2, stream)));
    if (unused) {
      k_rb_count_entries<<<1, 64, 0, s>>>(N, nsrcs, unused);
      HIPCHK(hipGetLastError());
    }
    return XDRG_OK;
  }
  auto *owner = static_cast<unsigned long long *>(d_workspace);
  auto *tiles = owner + rb_ws_owner(n) / 8;
  auto *won = tiles + rb_ws_tiles(n) / 8;
  k_rb_fill<<<uint32_t(nb), kRbThreads, 0, s>>>(owner, n);
  HIPCHK(hipGetLastError());
  if (cblocks) {
    k_rb_claim<<<uint32_t(cblocks), kRbThreads, 0, s>>>(d_hdrs, n, C, nsrcs, owner);
    HIPCHK(hipGetLastError());
  }
  k_rb_sizes<<<uint32_t(nb), kRbThreads, 0, s>>>(d_hdrs, n, owner, P, tiles, won);
  HIPCHK(hipGetLastError());
  k_rb_scan<<<1, 1024, 0, s>>>(tiles, won, nb, N, nsrcs, d_offsets + n, d_status, unused);
  HIPCHK(hipGetLastError());
  auto *err = reinterpret_cast<unsigned long long *>(&d_status->first_error);
  uint8_t *out = static_cast<uint8_t *>(d_out);
  if (copy_width() == 4)
    k_rb_emit<4><<<uint32_t(nb), kRbThreads, 0, s>>>(d_hdrs, n, owner, P, out, out_capacity, d_offsets, tiles, err);
  else
    k_rb_emit<16><<<uint32_t(nb), kRbThreads, 0, s>>>(d_hdrs, n, owner, P, out, out_capacity, d_offsets, tiles, err);
  HIPCHK(hipGetLastError());
  return XDRG_OK;
}

}  // extern "C"
