// Host helpers shared by the launchers of the RPC stages (rpc.hip, verify.hip,
// replies.hip, reply_batch.hip, call_batch.hip, settle.hip): argument checks,
// workspace layout and the source tables of batch_kernels.h.
#pragma once
#include <hip/hip_runtime.h>

#include "batch_kernels.h"
#include "plan.h"

#define HIPCHK(x)                                                             \
  do {                                                                        \
    hipError_t e_ = (x);                                                      \
    if (e_ != hipSuccess) return xdrg::record_hip_error(int(e_), #x);         \
  } while (0)

namespace xdrg {
namespace host {

inline bool misaligned(const void *p, uintptr_t mask) { return reinterpret_cast<uintptr_t>(p) & mask; }

// [a, a + an) and [b, b + bn) share a byte
inline bool overlap(const void *a, uint64_t an, const void *b, uint64_t bn) {
  const uintptr_t x = reinterpret_cast<uintptr_t>(a), y = reinterpret_cast<uintptr_t>(b);
  return an && bn && x < y + bn && y < x + an;
}

inline size_t align256(size_t v) { return (v + 255) / 256 * 256; }

// ------------------------------------------------------------- workspaces
inline uint64_t tiles_of(uint64_t n) { return (n + dev::kTileThreads - 1) / dev::kTileThreads; }
// one word per tile and one more (the gathers and the streams), 256-byte aligned
inline size_t ws_tiles(uint64_t n) { return align256((tiles_of(n) + 1) * 8); }
// a gather: tile counts, then tile bytes
inline size_t gather_ws_bytes(uint64_t n) { return 2 * ws_tiles(n); }
// a stream built from sources: owner words (n), then per tile the message
// bytes and the winners
inline size_t ws_owner(uint64_t n) { return align256(n * 8); }
inline size_t stream_ws_bytes(uint64_t n) { return ws_owner(n) + 2 * ws_tiles(n); }

// ----------------------------------------------------------------- sources
// S: xdrg_rpc_result_src or xdrg_rpc_arg_src (the fields they share).
template <class S>
bool valid_srcs(const S *srcs, uint32_t nsrcs) {
  for (uint32_t k = 0; k < nsrcs; ++k) {
    const S &s = srcs[k];
    if (s.count_cap && !s.d_index) return false;
    if (!s.d_bytes && s.fixed_size) return false;
    if (s.d_bytes && !s.d_offsets && (!s.fixed_size || (s.fixed_size & 3u))) return false;
  }
  return true;
}
template <class S>
bool misaligned_srcs(const S *srcs, uint32_t nsrcs) {
  for (uint32_t k = 0; k < nsrcs; ++k)
    if (misaligned(srcs[k].d_bytes, 3) || misaligned(srcs[k].d_offsets, 7) || misaligned(srcs[k].d_index, 7) ||
        misaligned(srcs[k].d_count, 7))
      return true;
  return false;
}

// The claim and count tables; each(k, srcs[k], offsets, fixed) fills the
// stage's own.  Returns the claim's workgroups (to be checked against the
// grid limit before the launch).
template <class S, class F>
uint64_t build_src_tables(const S *srcs, uint32_t nsrcs, dev::src_claim_table &C, dev::src_count_table &N, F &&each) {
  uint64_t cblocks = 0;
  for (uint32_t k = 0; k < nsrcs; ++k) {
    const S &s = srcs[k];
    const bool has = s.d_bytes != nullptr;  // no bytes (void results, no arguments): every span is [0, 0)
    const uint64_t *offs = has ? s.d_offsets : nullptr;
    const uint32_t fixed = has ? s.fixed_size : 0u;
    C.e[k] = dev::src_claim{s.d_index, s.d_count, offs, s.bytes_len, s.count_cap, fixed};
    N.count[k] = s.d_count;
    N.cap[k] = s.count_cap;
    C.blk[k] = uint32_t(cblocks);
    cblocks += tiles_of(s.count_cap);
    each(k, s, offs, fixed);
  }
  for (uint32_t k = nsrcs; k <= dev::kMaxSrcs; ++k) C.blk[k] = uint32_t(cblocks);
  return cblocks;
}

}  // namespace host
}  // namespace xdrg
