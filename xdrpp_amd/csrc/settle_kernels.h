// Settling a reply batch (settle.hip): what the asynchronous client's pending
// calls became, and calls_ after the erases.  rpc_sock::recv_msg erases a call
// at its first reply (xdrpp/msgsock.cc:217-219), the callback of
// asynchronous_client_base::invoke receives rpc_call_stat(hdr)
// (xdrpp/rpc_msg.cc:69-90, the catch of arpc.h:87-89), and abort_all_calls
// hands every call still outstanding NETWORK_ERROR (msgsock.cc:190-200,
// arpc.h:60-61).
//
//   k_st_call_stats  one lane per table entry: its rpc_call_stat from the
//                    header of the message that answers it
//   k_st_count       the kept entries (no reply) of every 256-entry tile
//                    (tile_reduce)
//   k_tile_scan<1, 1, count_total>   exclusive scan in place of the tile
//                    counts; the total to *count (also with no tile at all:
//                    an empty table still gets its 0 from here)
//   k_st_scatter     one lane per entry: its rank is the kept lanes below it
//                    in its wave's ballot, plus the waves before it in the
//                    tile (LDS), plus the tile's base; kept entries leave as
//                    consecutive 8-byte stores in table order
//
// No atomic anywhere: the order is the table's, and the result is a function
// of the inputs only.
#pragma once
#include "batch_kernels.h"

namespace xdrg {
namespace dev {

// ------------------------------------------------------------- call stats
// rpc_call_stat(hdr) (rpc_msg.cc:69-90) after xdrg_rpc_verify_results: every
// action a matched reply cannot carry is GARBAGE_RES, as is a reply_of that
// names no message of this batch (no header is read for it).
__global__ __launch_bounds__(kTileThreads) void k_st_call_stats(const xdrg_rpc_hdr *__restrict__ hdrs, uint64_t n,
                                                              const uint64_t *__restrict__ reply_of,
                                                              uint64_t ncalls, uint32_t unanswered,
                                                              xdrg_rpc_call_stat *__restrict__ stats) {
  const uint64_t c = static_cast<uint64_t>(blockIdx.x) * kTileThreads + threadIdx.x;
  if (c >= ncalls) return;
  const uint64_t i = reply_of[c];
  xdrg_rpc_call_stat s = {XDRG_RPCS_GARBAGE_RES, 0u};
  if (i == XDRG_RPC_NO_CALL) {
    s.type = unanswered;
  } else if (i < n) {
    const xdrg_rpc_hdr &h = hdrs[i];
    const uint32_t a = h.action;
    if (a == XDRG_RPCR_OK) {
      s.type = XDRG_RPCS_ACCEPT_STAT;
    } else if (a == XDRG_RPCR_ACCEPT_STAT) {
      s.type = XDRG_RPCS_ACCEPT_STAT;
      s.stat = h.w[XDRG_RPC_W_STAT];
    } else if (a == XDRG_RPCR_AUTH_STAT) {
      s.type = XDRG_RPCS_AUTH_STAT;
      s.stat = h.w[XDRG_RPC_W_WHY];
    } else if (a == XDRG_RPCR_RPCVERS_MISMATCH) {
      s.type = XDRG_RPCS_RPCVERS_MISMATCH;
    }
  }
  stats[c] = s;
}

// ---------------------------------------------------------------- retire
__global__ __launch_bounds__(kTileThreads) void k_st_count(const uint64_t *__restrict__ reply_of, uint64_t ncalls,
                                                         unsigned long long *__restrict__ tile_kept) {
  const uint64_t j = static_cast<uint64_t>(blockIdx.x) * kTileThreads + threadIdx.x;
  tile_reduce(0, j < ncalls && reply_of[j] == XDRG_RPC_NO_CALL, nullptr, tile_kept);
}

// A kept entry's rank is at most its own position (the entries before it that
// are kept), so every store stays below ncalls; the compare keeps it there
// even when reply_of changes between the passes.
__global__ __launch_bounds__(kTileThreads) void k_st_scatter(const xdrg_rpc_call *__restrict__ calls, uint64_t ncalls,
                                                           const uint64_t *__restrict__ reply_of,
                                                           const unsigned long long *__restrict__ tile_base,
                                                           xdrg_rpc_call *__restrict__ kept,
                                                           uint64_t *__restrict__ kept_pos) {
  __shared__ uint32_t wk[kTileThreads / 64];
  const uint32_t tid = threadIdx.x, lane = tid & 63u, wid = tid >> 6;
  const uint64_t j = static_cast<uint64_t>(blockIdx.x) * kTileThreads + tid;
  const bool keep = j < ncalls && reply_of[j] == XDRG_RPC_NO_CALL;
  const unsigned long long m = __ballot(keep);
  if (lane == 0u) wk[wid] = __popcll(m);
  __syncthreads();
  uint64_t rank = tile_base[blockIdx.x] + __popcll(m & ((1ull << lane) - 1ull));
  for (uint32_t k = 0; k < wid; ++k) rank += wk[k];
  if (j >= ncalls) return;
  const bool put = keep && rank < ncalls;
  if (put) kept[rank] = calls[j];
  if (kept_pos) kept_pos[j] = put ? rank : XDRG_RPC_NO_CALL;
}

}  // namespace dev
}  // namespace xdrg
