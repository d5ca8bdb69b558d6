// The asynchronous client's send half for a whole batch (call_batch.hip):
// asynchronous_client_base::invoke (xdrpp/arpc.h:41-59) takes an xid from
// rpc_sock::get_xid (msgsock.h:118-122), marshals xdr_to_msg(hdr, args...)
// and rpc_sock::send_call (msgsock.cc:227-232) remembers the call.  Here the
// arguments come as sources (what xdrg_encode wrote for one procedure, and
// the call position of each of them) and the batch's calls leave as one
// record-marked stream in call order.
//
//   k_cb_next_xids    one lane per xid: the (k+1)-th value after last_xid that
//                     is not pending, by two binary searches of the table
//                     (pending_kernels.h)
//   k_owner_fill, k_src_claim<cb_usable>   the lowest usable entry that names
//                     a position owns it (batch_kernels.h)
//   k_cb_sizes        one lane per position: its message bytes (44 + L with a
//                     winning entry, else 0) and whether an entry won it, both
//                     summed per 256-position tile
//   k_tile_scan<1, 2, stream_totals>   exclusive scan of the tile bytes; the
//                     total; counts[0] = n - the winners, counts[1] = the
//                     sources' entries - the winners
//   k_cb_emit         offsets and d_sent a lane per position; the bytes a wave
//                     per run of 64 positions (stretch_write, W = 16).  The
//                     mark and the ten header words come from LDS, the argument
//                     bytes from the winning source.
//   k_cb_pending_add  one lane per old and per new entry of the pending table:
//                     its place in the merged table by binary searches
//                     (pending_kernels.h)
#pragma once
#include "pending_kernels.h"

namespace xdrg {
namespace dev {

constexpr uint32_t kCbHdrWords = 11;  // mark + the call header (arpc.h:44-48: xid, CALL, 2, prog, vers, proc, cred, verf)

// What the sizes need of a source: how long a winning entry is.
struct cb_size_src {
  const uint64_t *offsets;
  uint64_t fixed;
};
struct cb_size_table {
  cb_size_src e[kMaxSrcs];
};

// What the emit needs: where a winning entry's bytes are, and the words its
// procedure puts into the header and the pending table.
struct cb_emit_src {
  const uint8_t *bytes;
  const uint64_t *offsets;
  uint32_t fixed, res;
  uint32_t prog, vers, proc, rsv;
};
struct cb_emit_table {
  cb_emit_src e[kMaxSrcs];
};
static_assert(sizeof(cb_emit_table) + 64 < 4096, "kernel arguments under 4 KiB");

// Every position takes an entry; a call is 40 bytes of header (and 4 of mark)
// before its arguments.
struct cb_usable {
  static constexpr uint32_t kHdrBytes = 40;
  __device__ __forceinline__ bool operator()(uint64_t) const { return true; }
};

// ---------------------------------------------- next xids, pending add
// rpc_sock::get_xid() n times, each followed by send_call (msgsock.h:118-122):
// pt_nth_free on the whole table.
__global__ __launch_bounds__(kPendingThreads) void k_cb_next_xids(const xdrg_rpc_call *__restrict__ calls,
                                                                  uint64_t ncalls, uint32_t last, uint64_t n,
                                                                  uint32_t *__restrict__ xids) {
  const uint64_t k = static_cast<uint64_t>(blockIdx.x) * kPendingThreads + threadIdx.x;
  if (k >= n) return;
  xids[k] = pt_nth_free(calls, ncalls, last, k);
}

// calls_ after the sends: lanes 0..ncalls-1 place the old entries, the next n
// the new ones.  Every position written is below ncalls + n whatever the
// arrays hold (a lower bound is at most its array's length).
__global__ __launch_bounds__(kPendingThreads) void k_cb_pending_add(const xdrg_rpc_call *__restrict__ calls,
                                                                    uint64_t ncalls,
                                                                    const xdrg_rpc_call *__restrict__ fresh,
                                                                    uint64_t n, xdrg_rpc_call *__restrict__ merged,
                                                                    uint64_t *__restrict__ old_pos,
                                                                    uint64_t *__restrict__ new_pos) {
  const uint64_t t = static_cast<uint64_t>(blockIdx.x) * kPendingThreads + threadIdx.x;
  if (t >= ncalls + n) return;
  const uint64_t w = n ? pt_wrap_point(fresh, n) : 0u;
  if (t < ncalls) {
    const xdrg_rpc_call c = calls[t];
    const uint64_t below = pt_fresh_below(fresh, n, w, c.xid);
    merged[t + below] = c;
    if (old_pos) old_pos[t] = t + below;
  } else {
    const uint64_t k = t - ncalls;
    const xdrg_rpc_call c = fresh[k];
    const uint64_t rank = k < w ? (n - w) + k : k - w;
    const uint64_t at = pt_lower_bound(calls, ncalls, c.xid) + rank;
    merged[at] = c;
    if (new_pos) new_pos[k] = at;
  }
}

// ------------------------------------------------------------ call stream
__global__ __launch_bounds__(kTileThreads) void k_cb_sizes(uint64_t n, const unsigned long long *__restrict__ owner,
                                                           const cb_size_table T,
                                                           unsigned long long *__restrict__ tile_bytes,
                                                           unsigned long long *__restrict__ tile_won) {
  const uint64_t i = static_cast<uint64_t>(blockIdx.x) * kTileThreads + threadIdx.x;
  unsigned long long t = 0;
  bool won = false;
  if (i < n) {
    const unsigned long long own = owner[i];
    won = own != kNoOwner;
    if (won) {
      uint64_t a, b;
      src_span(T.e[owner_src(own)], owner_pos(own), &a, &b);
      t = 4u * kCbHdrWords + (b - a);  // the claim has checked the span
    }
  }
  tile_reduce(t, won, tile_bytes, tile_won);
}

// Every message starts with its column's eleven words.
using cb_wave_lds = wave_stretch<kCbHdrWords, false>;

__global__ __launch_bounds__(kTileThreads) void k_cb_emit(const uint32_t *__restrict__ xids, uint64_t n,
                                                          const unsigned long long *__restrict__ owner,
                                                          const cb_emit_table T, uint8_t *__restrict__ out,
                                                          uint64_t cap, uint64_t *__restrict__ offsets,
                                                          xdrg_rpc_call *__restrict__ sent,
                                                          const unsigned long long *__restrict__ tile_bytes,
                                                          unsigned long long *err) {
  __shared__ cb_wave_lds lds[kTileThreads / 64];
  const uint32_t tid = threadIdx.x, lane = tid & 63u, wid = tid >> 6;
  const uint64_t i = static_cast<uint64_t>(blockIdx.x) * kTileThreads + tid;
  cb_wave_lds &L = lds[wid];
  uint32_t bytes = 0;
  const uint8_t *src = nullptr;
  if (i < n) {
    const uint32_t xid = xids[i];
    const unsigned long long own = owner[i];
    uint32_t res = XDRG_RPC_RES_UNSENT;
    if (own != kNoOwner) {
      const cb_emit_src S = T.e[owner_src(own)];
      uint64_t a, b;
      src_span(S, owner_pos(own), &a, &b);
      src = S.bytes + a;
      bytes = 4u * kCbHdrWords + static_cast<uint32_t>(b - a);
      res = S.res;
      // message_t::alloc mark (marshal.cc:15-31), then rpc_msg's words (arpc.h:44-48)
      L.w[0][lane] = mark_word(bytes - 4u);
      L.w[1][lane] = bswap32(xid);
      L.w[2][lane] = 0u;  // CALL
      L.w[3][lane] = bswap32(2u);
      L.w[4][lane] = bswap32(S.prog);
      L.w[5][lane] = bswap32(S.vers);
      L.w[6][lane] = bswap32(S.proc);
      L.w[7][lane] = 0u;  // cred: AUTH_NONE, body<>
      L.w[8][lane] = 0u;
      L.w[9][lane] = 0u;  // verf
      L.w[10][lane] = 0u;
    }
    if (sent) sent[i] = xdrg_rpc_call{xid, res};
  }
  const stretch_at p = stretch_place(bytes, bytes != 0u, i, tile_bytes, cap, err, L.end, [&](uint64_t at) {
    if (i < n) offsets[i] = at;
  });
  L.src[lane] = src;
  __syncthreads();
  stretch_write<16>(L, out + p.wbase, lane);
}

}  // namespace dev
}  // namespace xdrg
