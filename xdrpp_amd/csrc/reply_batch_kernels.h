// The server's reply step for a whole dispatched batch (reply_batch.hip):
// srpc_server::run (xdrpp/srpc.cc:83-88) writes one reply per answered call in
// call order -- xdr_to_msg(rpc_success_hdr(xid), *res) (srpc.h:152,
// server.h:27-49) for a call its handler served, one of the rpc_*_msg error
// replies (server.cc:8-67) for a call that failed.  Here the results come as
// sources (what xdrg_encode wrote, and the message each result answers) and
// the batch's replies leave as one record-marked stream in message order.
// The stages are those of batch_kernels.h:
//
//   k_owner_fill, k_src_claim<rb_usable>   the lowest usable entry that
//                answers a DISPATCH owns it
//   k_rb_sizes   one lane per message: its reply bytes (error reply by action,
//                28 + L for a DISPATCH with a winning entry, else 0) and
//                whether an entry won it, both summed per 256-message tile
//   k_tile_scan<1, 2, stream_totals>   exclusive scan of the tile bytes; the
//                total; *unused = the sources' entries - the winners (no
//                atomic on one word: 16K waves adding to *unused cost more
//                than the copy)
//   k_rb_emit    offsets a lane per message; the bytes a wave per run of 64
//                messages (stretch_write, W = 4 or 16).  The words of an error
//                reply and words 0..6 of a success reply come from LDS, the
//                result bytes from the winning source.
#pragma once
#include "batch_kernels.h"

namespace xdrg {
namespace dev {

constexpr uint32_t kRbHdrWords = 7;  // mark + rpc_success_hdr (server.h:27-49)
constexpr uint32_t kRbMaxWords = 9;  // the longest error reply (PROG_MISMATCH)

// What the sizes and the emit need of a source: where a winning entry's bytes
// are.
struct rb_span_src {
  const uint8_t *bytes;
  const uint64_t *offsets;
  uint64_t fixed;
};
struct rb_span_table {
  rb_span_src e[kMaxSrcs];
};
static_assert(sizeof(rb_span_table) + 128 < 4096, "kernel arguments under 4 KiB");

// Only a DISPATCH takes a result; a success reply is 24 bytes of mark and
// header around it.
struct rb_usable {
  static constexpr uint32_t kHdrBytes = 24;
  const xdrg_rpc_hdr *hdrs;
  __device__ __forceinline__ bool operator()(uint64_t i) const { return hdrs[i].action == XDRG_RPC_DISPATCH; }
};

// Message bytes (mark included) of a header's error reply (server.cc:8-67).
__device__ __forceinline__ uint32_t rb_error_bytes(uint32_t action) {
  switch (action) {
    case XDRG_RPC_RPC_MISMATCH:
    case XDRG_RPC_PROG_UNAVAIL:
    case XDRG_RPC_PROC_UNAVAIL:
    case XDRG_RPC_GARBAGE_ARGS:
    case XDRG_RPC_SYSTEM_ERR: return 28;
    case XDRG_RPC_PROG_MISMATCH: return 36;
    case XDRG_RPC_AUTH_ERROR: return 24;
    default: return 0;
  }
}

// The reply of message i: its bytes, and for a success reply where the result
// bytes are (*src; owner decides, the claim has checked the span).
__device__ __forceinline__ uint32_t rb_reply(uint32_t action, unsigned long long own, const rb_span_table &T,
                                             const uint8_t **src) {
  *src = nullptr;
  if (action != XDRG_RPC_DISPATCH) return rb_error_bytes(action);
  if (own == kNoOwner) return 0u;  // an asynchronous service that has not answered yet
  const rb_span_src S = T.e[owner_src(own)];
  uint64_t a, b;
  src_span(S, owner_pos(own), &a, &b);
  *src = S.bytes + a;
  return 4u * kRbHdrWords + static_cast<uint32_t>(b - a);
}

__global__ __launch_bounds__(kTileThreads) void k_rb_sizes(const xdrg_rpc_hdr *__restrict__ hdrs, uint64_t n,
                                                           const unsigned long long *__restrict__ owner,
                                                           const rb_span_table T,
                                                           unsigned long long *__restrict__ tile_bytes,
                                                           unsigned long long *__restrict__ tile_won) {
  const uint64_t i = static_cast<uint64_t>(blockIdx.x) * kTileThreads + threadIdx.x;
  unsigned long long t = 0;
  bool won = false;
  if (i < n) {
    const uint32_t action = hdrs[i].action;
    const unsigned long long own = action == XDRG_RPC_DISPATCH ? owner[i] : kNoOwner;
    const uint8_t *src;
    t = rb_reply(action, own, T, &src);
    won = own != kNoOwner;
  }
  tile_reduce(t, won, tile_bytes, tile_won);
}

// A message's reply starts with nw of its column's words: 7 for a success
// reply, then the result; all of an error reply's.
using rb_wave_lds = wave_stretch<kRbMaxWords, true, kRbHdrWords>;

template <int W>
__global__ __launch_bounds__(kTileThreads) void k_rb_emit(const xdrg_rpc_hdr *__restrict__ hdrs, uint64_t n,
                                                          const unsigned long long *__restrict__ owner,
                                                          const rb_span_table T, uint8_t *__restrict__ out,
                                                          uint64_t cap, uint64_t *__restrict__ offsets,
                                                          const unsigned long long *__restrict__ tile_bytes,
                                                          unsigned long long *err) {
  __shared__ rb_wave_lds lds[kTileThreads / 64];
  const uint32_t tid = threadIdx.x, lane = tid & 63u, wid = tid >> 6;
  const uint64_t i = static_cast<uint64_t>(blockIdx.x) * kTileThreads + tid;
  rb_wave_lds &L = lds[wid];
  uint32_t bytes = 0, nw = 0;
  const uint8_t *src = nullptr;
  if (i < n) {
    const xdrg_rpc_hdr *h = hdrs + i;
    const u32x4 q = *reinterpret_cast<const u32x4 *>(h);  // xid, action | err | mtype, w[0], w[1]
    const uint32_t action = q.y & 0xffffu;
    const unsigned long long own = action == XDRG_RPC_DISPATCH ? owner[i] : kNoOwner;
    bytes = rb_reply(action, own, T, &src);
    if (bytes) {
      // message_t::alloc mark (marshal.cc:15-31), then the xdr_put words
      uint32_t w3 = 0 /* MSG_ACCEPTED */, w4 = 0 /* AUTH_NONE */, w5 = 0 /* body<> */, w6 = 0 /* SUCCESS */;
      uint32_t w7 = 0, w8 = 0;
      if (action == XDRG_RPC_RPC_MISMATCH) {  // rpc_rpc_mismatch_msg, server.cc:55-68
        w3 = 1 /* MSG_DENIED */; w4 = 0 /* RPC_MISMATCH */; w5 = 2; w6 = 2;
      } else if (action == XDRG_RPC_AUTH_ERROR) {  // rpc_auth_error_msg, server.cc:41-53
        w3 = 1 /* MSG_DENIED */; w4 = 1 /* AUTH_ERROR */; w5 = h->w[XDRG_RPC_W_WHY];
      } else if (action != XDRG_RPC_DISPATCH) {  // rpc_accepted_error_msg / rpc_prog_mismatch_msg, server.cc:8-39
        w6 = action == XDRG_RPC_PROG_UNAVAIL  ? 1u
           : action == XDRG_RPC_PROG_MISMATCH ? 2u
           : action == XDRG_RPC_PROC_UNAVAIL  ? 3u
           : action == XDRG_RPC_GARBAGE_ARGS  ? 4u
                                              : 5u /* SYSTEM_ERR */;
        if (action == XDRG_RPC_PROG_MISMATCH) { w7 = h->w[XDRG_RPC_W_LOW]; w8 = h->w[XDRG_RPC_W_HIGH]; }
      }
      nw = action == XDRG_RPC_DISPATCH ? kRbHdrWords : bytes / 4u;
      L.w[0][lane] = mark_word(bytes - 4u);
      L.w[1][lane] = bswap32(q.x);
      L.w[2][lane] = bswap32(1u /* REPLY */);
      L.w[3][lane] = bswap32(w3);
      L.w[4][lane] = bswap32(w4);
      L.w[5][lane] = bswap32(w5);
      L.w[6][lane] = bswap32(w6);
      L.w[7][lane] = bswap32(w7);
      L.w[8][lane] = bswap32(w8);
    }
  }
  const stretch_at p = stretch_place(bytes, bytes != 0u, i, tile_bytes, cap, err, L.end, [&](uint64_t at) {
    if (i < n) offsets[i] = at;
  });
  L.src[lane] = src;
  L.nw[lane] = nw;
  __syncthreads();
  stretch_write<W>(L, out + p.wbase, lane);
}

}  // namespace dev
}  // namespace xdrg
